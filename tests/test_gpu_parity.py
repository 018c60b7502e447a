"""GPU parity tests: the HIP path (through the C-ABI of libminigpt4.so) against the CPU oracle on the same seeded inputs.

Tolerances (north_star: greedy token ids identical; logits within 1e-2 relative):
  * activation quantisation (Q8_K / Q8_0): bit-exact int8 / scales;
  * quantised mat-mul: integer block dots are exact, only the fp32 summation order differs -> 2e-5 relative to the row maximum;
  * f16 MFMA GEMM: exact products, fp32 accumulation order differs -> 2e-5 relative;
  * whole-model logits of the tiny (conditioned) models here: LOGIT_TOL = 1e-2 of the largest |logit| (north_star) and 2 x the recorded observation, 3e-3 for f16 weights
    (no int8 step); free-running greedy ids identical at every step.  Bit-identical logits in parity mode: tests/test_gpu_paritymode.py.  Headline sizes:
    tests/test_gpu_headline.py (observed errors in tests/golden/parity_observed.json).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QTYPES = ["q4_0", "q4_1", "q5_0", "q5_1", "q8_0", "q2_k", "q4_k", "q5_k", "q6_k", "f16", "f32"]


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def test_device_present(gpu_lib):
    assert gpu_lib.amd_device_count() >= 1


@pytest.mark.parametrize("rms", [False, True])
def test_activation_quantisation_bit_exact(gpu_lib, rms):
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    rng = np.random.default_rng(5)
    N, K = 3, 1024
    x = (rng.standard_normal((N, K)) * 0.7).astype(np.float32)
    x[1, 256:512] = 0.0                       # an all-zero Q8_K block
    x[0, 10] = 3.0
    x[0, 200] = -3.0                          # +/- tie for the block maximum: the first one decides the sign of the scale
    w = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32) if rms else None
    q8k, dk, bs, q80, d0 = gpu_lib.amd_test_quantize(x, w)
    y = x
    if rms:
        y = np.empty_like(x)
        for t in range(N):
            s = np.float64(0)
            for v in x[t]:
                s += np.float64(np.float32(v * v))
            scale = np.float32(1.0) / np.sqrt(np.float32(np.float32(s / K) + np.float32(1e-6)), dtype=np.float32)
            y[t] = (x[t] * scale) * w
    for t in range(N):
        ref = R.quantize_row(Q.GGML_Q8_K, y[t]).reshape(K // 256, 292)
        assert np.array_equal(ref[:, 0:4].copy().view(np.float32).reshape(-1), dk[t])
        assert np.array_equal(ref[:, 4:260].copy().view(np.int8).reshape(-1), q8k[t])
        assert np.array_equal(ref[:, 260:292].copy().view(np.int16).reshape(-1), bs[t])
        ref0 = R.quantize_row(Q.GGML_Q8_0, y[t]).reshape(K // 32, 34)
        assert np.array_equal(ref0[:, 2:].copy().view(np.int8).reshape(-1), q80[t])
        assert np.array_equal(ref0[:, 0:2].copy().view(np.float16).astype(np.float32).reshape(-1), d0[t])


@pytest.mark.parametrize("wtype", QTYPES)
@pytest.mark.parametrize("shape", [(1, 512, 96), (5, 768, 70), (1, 5120, 64), (33, 768, 70), (70, 1024, 130), (142, 2048, 256),    # N >= 16: int8-MFMA prefill path
                                   (257, 352, 100), (40, 1408, 64)])     # the ViT's row lengths (11 / 44 blocks of 32; 32-element block types only)
def test_mul_mat_matches_oracle(gpu_lib, wtype, shape):
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    N, n_in, n_out = shape
    t = Q.NAME_TO_TYPE[wtype]
    if n_in % Q.BLOCK[t][0]:
        pytest.skip("row length is not a whole number of blocks of this type")
    rng = np.random.default_rng(sum(map(ord, wtype)) * 1000 + sum(shape))
    w = (0.05 * rng.standard_normal((n_out, n_in))).astype(np.float32)
    raw = Q.quantize(t, w)
    x = rng.standard_normal((N, n_in)).astype(np.float32)
    want = R.mul_mat(t, raw, n_in, n_out, x)
    got = gpu_lib.amd_test_mul_mat(t, raw, n_in, n_out, x)
    assert got.shape == want.shape
    assert _rel(got, want) < 2e-5, (wtype, shape, _rel(got, want))
    # sanity vs float64 on the dequantised weights: within activation-quantisation noise
    f64 = x.astype(np.float64) @ Q.dequantize(t, raw, w.size).reshape(n_out, n_in).T
    assert _rel(got, f64) < 3e-2


def _prepared_row(prep, x, x2, silu_tab):
    """The activation row a decode mat-vec consumes, computed the way ggml does (fp32 ops, double sum of squares, fp16 SiLU table)."""
    if prep == 1:
        s = np.float64(0)
        for v in x:
            s += np.float64(np.float32(v * v))
        scale = np.float32(1.0) / np.sqrt(np.float32(np.float32(s / len(x)) + np.float32(1e-6)), dtype=np.float32)
        return (x * scale) * x2
    if prep == 3:
        return silu_tab[x.astype(np.float16).view(np.uint16)].astype(np.float32) * x2
    return x


def _silu_table():
    import refcpu as R
    return R.table(1).view(np.float16)          # uint16 bit patterns of ggml's table_silu_f16


# (type, K): K / 32 / 64 = units per lane: 1, 2, 3, 6, 7 -> every register-tiling of the persistent-wave kernel; rows > 2048 waves -> several groups per wave
MATVEC_CASES = [("q4_0", 512), ("q5_k", 512), ("q4_1", 4096), ("q4_k", 4096), ("q5_0", 5120), ("q5_k", 5120), ("q6_k", 5120), ("q5_1", 5120), ("q4_0", 11008),
                ("q4_k", 11008), ("q5_k", 13824), ("q6_k", 13824),
                # round 5: Q8_0 / F16 rows on the same pipelined kernel (16-byte units of 16 / 8 weights: 1, 4, 5, 11 resp. 1, 2, 8, 10 units per lane; 2048 and 1024 take
                # the next larger instantiation with masked surplus units) -- the real Vicuna-v0 file's F16 output matrix, the 7B Q8_0 file
                ("q8_0", 512), ("q8_0", 2048), ("q8_0", 4096), ("q8_0", 5120), ("q8_0", 11008), ("f16", 256), ("f16", 1024), ("f16", 2040), ("f16", 4096), ("f16", 5120)]


@pytest.mark.parametrize("wtype,K", MATVEC_CASES)
@pytest.mark.parametrize("prep,fuse", [(2, False), (1, True), (2, True), (3, True), (1, False)])
def test_decode_matvec_variants_match_oracle(gpu_lib, wtype, K, prep, fuse):
    """The decode path's own kernel (k_matvec_v2; amd_test_mul_mat exercises the prefill kernels): 1 / 3 matrices per launch, standalone and
    in-prologue activation preparation, residual add -- against the oracle's quantise + mul_mat on the identically prepared row."""
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    rng = np.random.default_rng(K * 7 + prep * 3 + int(fuse) + sum(map(ord, wtype)))
    n_mat = 3 if prep == 1 else 1
    rows = 2300 if K <= 5120 else 1100           # > 2048 waves x 1 row for the small K, ragged against the wave count for all
    w = (0.03 * rng.standard_normal((n_mat * rows, K))).astype(np.float32)
    raw = Q.quantize(t, w)
    x = (rng.standard_normal(K) * (3.0 if prep == 3 else 1.0)).astype(np.float32)
    x2 = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32) if prep != 2 else None
    res = rng.standard_normal(n_mat * rows).astype(np.float32) if prep == 2 else None
    got = gpu_lib.amd_test_matvec(t, raw, n_mat, K, rows, x, x2, prep=prep, fuse=fuse, residual=res).reshape(-1)
    row = _prepared_row(prep, x, x2, _silu_table())
    want = R.mul_mat(t, raw, K, n_mat * rows, row[None, :])[0]
    if res is not None:
        want = want + res
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max(), (wtype, K, prep, fuse)


@pytest.mark.parametrize("wtype,K", [("q5_k", 512), ("q4_0", 4096), ("q4_k", 4096), ("q5_k", 5120), ("q6_k", 5120)])
@pytest.mark.parametrize("fuse", [False, True])
def test_decode_matvec_silu_pair_epilogue(gpu_lib, wtype, K, fuse):
    """w1|w3 in one launch writing silu(w1 x) * (w3 x): equals the oracle's two mat-vecs pushed through the fp16 SiLU table."""
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    rng = np.random.default_rng(K + int(fuse))
    rows = 2500
    w = (0.05 * rng.standard_normal((2 * rows, K))).astype(np.float32)
    raw = Q.quantize(t, w)
    x = rng.standard_normal(K).astype(np.float32)
    nw = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32)
    got = gpu_lib.amd_test_matvec(t, raw, 2, K, rows, x, nw, prep=1, fuse=fuse, epi=1).reshape(-1)
    ab = R.mul_mat(t, raw, K, 2 * rows, _prepared_row(1, x, nw, None)[None, :])[0]
    tab = _silu_table()
    want = tab[ab[:rows].astype(np.float16).view(np.uint16)].astype(np.float32) * ab[rows:]
    # the table index is the fp16 rounding of a value that itself carries 2e-5 of summation-order noise: allow a neighbouring table entry
    assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max()
    assert np.mean(np.abs(got - want) <= 2e-5 * np.abs(want).max()) > 0.97


@pytest.mark.parametrize("t1,K", [("q5_k", 5120), ("q4_k", 4096), ("q5_k", 512), ("q4_k", 8192)])
@pytest.mark.parametrize("fuse", [False, True])
def test_decode_matvec_mixed_types_one_launch(gpu_lib, t1, K, fuse):
    """wq|wk (Q4_K / Q5_K) and a Q6_K wv (llama.cpp's "more bits" layers) streamed by one launch."""
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    ta, tb = Q.NAME_TO_TYPE[t1], Q.NAME_TO_TYPE["q6_k"]
    rng = np.random.default_rng(K * 3 + int(fuse))
    rows = 1500
    wa = (0.03 * rng.standard_normal((2 * rows, K))).astype(np.float32)
    wb = (0.03 * rng.standard_normal((rows, K))).astype(np.float32)
    ra, rb = Q.quantize(ta, wa), Q.quantize(tb, wb)
    x = rng.standard_normal(K).astype(np.float32)
    nw = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32)
    got = gpu_lib.amd_test_matvec(ta, ra, 2, K, rows, x, nw, prep=1, fuse=fuse, type2=tb, raw2=rb).reshape(-1)
    row = _prepared_row(1, x, nw, None)[None, :]
    want = np.concatenate([R.mul_mat(ta, ra, K, 2 * rows, row)[0], R.mul_mat(tb, rb, K, rows, row)[0]])
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()


@pytest.mark.parametrize("shape", [(257, 176, 528), (32, 768, 100), (256, 592, 176), (70, 48, 33),
                                   (512, 1408, 256), (640, 704, 130), (1028, 6144, 384), (513, 64, 128)])   # M >= 512: the 128x128 LDS-DMA kernel (ragged M / N, one and many k tiles)
@pytest.mark.parametrize("gelu", [False, True])
def test_gemm_f16_mfma(gpu_lib, shape, gelu):
    import refcpu as R
    M, K, N = shape
    rng = np.random.default_rng(M * 7 + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (0.1 * rng.standard_normal((N, K))).astype(np.float32)   # asymmetric on purpose (catches a transposed C write)
    b = rng.standard_normal(N).astype(np.float32)
    got = gpu_lib.amd_test_gemm_f16(A, W, b, gelu)
    ref = A.astype(np.float16).astype(np.float64) @ W.astype(np.float16).astype(np.float64).T + b
    if gelu:
        tab = R.table(0).view(np.float16)
        ref32 = (A.astype(np.float16).astype(np.float64) @ W.astype(np.float16).astype(np.float64).T).astype(np.float32) + b
        want = tab[ref32.astype(np.float16).view(np.uint16)].astype(np.float32)
        # the fp16 rounding of the GELU argument can flip by one ulp where the fp32 sums differ in the last bits
        bad = np.abs(got - want) > 2e-3 * (1 + np.abs(want))
        assert bad.mean() < 1e-3
    else:
        assert _rel(got, ref) < 2e-5


GEMM_ARMS = [3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 38, 39]


@pytest.mark.parametrize("arm", GEMM_ARMS)
def test_gemm_f16_tile_shapes_are_bit_identical(gpu_lib, arm):
    """Every tile shape of the small-M fp16 GEMM (register-staged k_gemm_f16 arms 3..14, LDS-DMA ring k_gemm_dma arms 20..31; vision_kernels.hip launch_gemm_f16_arm)
    (arms 32..39: the 128x128 / 256x128 / 256x256 tiles of the large-M and F16 set launches) accumulates an output element over k in the same order, so on ragged shapes (M = 257, N not a tile multiple, one and several k tiles) each arm must reproduce the default
    launch bit for bit, GELU epilogue included; a shape outside an arm's range (K % 64) falls back to the default and is trivially equal."""
    import ctypes
    L = gpu_lib.library
    L.minigpt4_amd_test_set_gemm_arm.argtypes = [ctypes.c_int, ctypes.c_int]
    L.minigpt4_amd_test_set_gemm_arm.restype = None
    rng = np.random.default_rng(arm)
    try:
        for (M, K, N, gelu) in [(257, 256, 352, False), (257, 1408, 224, True), (70, 128, 96, False), (33, 592, 64, False), (300, 640, 1056, True)]:
            A = rng.standard_normal((M, K)).astype(np.float32)
            W = (0.1 * rng.standard_normal((N, K))).astype(np.float32)
            b = rng.standard_normal(N).astype(np.float32)
            L.minigpt4_amd_test_set_gemm_arm(-2, 0)                  # the 64x64 launch, whatever the shape
            want = gpu_lib.amd_test_gemm_f16(A, W, b, gelu)
            L.minigpt4_amd_test_set_gemm_arm(0, 0)                   # the launcher's own choice of tile shape
            assert np.array_equal(gpu_lib.amd_test_gemm_f16(A, W, b, gelu).view(np.uint32), want.view(np.uint32))
            L.minigpt4_amd_test_set_gemm_arm(arm, 0)
            got = gpu_lib.amd_test_gemm_f16(A, W, b, gelu)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (arm, M, K, N, float(np.abs(got - want).max()))
    finally:
        L.minigpt4_amd_test_set_gemm_arm(0, 0)


def test_encode_image_matches_oracle(gpu_lib, tiny_files):
    import refcpu as R
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G
    vp, llm = tiny_files
    ctx = gpu_lib.minigpt4_model_load(vp, llm("q4_0"), verbosity=1, n_ctx=64, n_batch=32)
    try:
        want_o = R.OracleVision(G.read_vision_file(vp))
        for seed in (42, 7):
            img = G.synth_image(seed)
            emb = gpu_lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(img))
            assert emb.n_embeddings == 32 * 4096
            got = np.ctypeslib.as_array(emb.data, shape=(emb.n_embeddings,)).copy().reshape(32, 4096)
            gpu_lib.minigpt4_free_embedding(emb)
            want = want_o.encode(img)
            assert _rel(got, want) < 2e-3, _rel(got, want)
        # error paths of the reference (minigpt4.cpp:2130-2138)
        bad = ML.array_to_image_struct(G.synth_image(1))
        bad.width = 100
        assert gpu_lib.library.minigpt4_encode_image(ctx.ptr, bad, ML.MiniGPT4Embedding(), 0) == 13
        bad = ML.array_to_image_struct(G.synth_image(1))
        bad.format = 2
        assert gpu_lib.library.minigpt4_encode_image(ctx.ptr, bad, ML.MiniGPT4Embedding(), 0) == 14
    finally:
        gpu_lib.minigpt4_free(ctx)


# Whole-model tolerance (north_star: "logits within 1e-2 relative", greedy ids identical).  The models of these tests are conditioned like the headline files
# (modelgen.TINY_CONDITIONED): on an i.i.d. Gaussian stack the reference arithmetic's own int8 re-roundings move the logits by percents of their range (measured:
# tests/test_cpu_host.py::test_oracle_sensitivity), which says nothing about a kernel.  Bit-level equality with the oracle is asserted in tests/test_gpu_paritymode.py;
# here the FAST kernels are held to 1e-2 of the largest |logit| AND to twice the error a GPU box recorded (tests/golden/parity_observed_tiny.json).
LOGIT_TOL = 1e-2


@pytest.mark.parametrize("wtype,mix", [("q4_0", "none"), ("q5_k", "q5_k_m"), ("q4_1", "none"), ("q8_0", "none"), ("q6_k", "none"), ("q5_0", "none"),
                                       ("q5_1", "none"), ("q4_k", "none"), ("f16", "none"), ("q2_k", "none")])
def test_llm_logits_and_greedy_tokens(gpu_lib, tiny_files, wtype, mix):
    import refcpu as R
    from conftest import observed_bar, record_observed
    from minigpt4_cpp_amd import modelgen as G
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=16)
    try:
        o = R.OracleLLM(G.read_llm_file(lp), n_ctx=96)
        toks = [1, 5, 300, 44, 270, 99, 400, 17, 33, 260, 301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311]   # 21 tokens: 2 chunks of n_batch=16
        gpu_lib.amd_eval_tokens(ctx, toks)
        o.eval_tokens(toks[:16])
        want = o.eval_tokens(toks[16:])
        got = gpu_lib.amd_logits(ctx)
        errs = [_rel(got, want)]
        # 24 FREE-RUNNING greedy steps (graph-replayed on the GPU): each side consumes its own greedy token, which must be the same one
        decided, ids = 0, []
        for _ in range(24):
            srt = np.sort(want)
            decided += int((srt[-1] - srt[-2]) / (np.abs(want).max() + 1e-30) > 2 * LOGIT_TOL)
            gid, oid = int(got.argmax()), int(want.argmax())
            assert gid == oid, (len(ids), gid, oid)
            ids.append(oid)
            gpu_lib.amd_eval_tokens(ctx, [gid])
            want = o.eval_tokens([oid])
            got = gpu_lib.amd_logits(ctx)
            errs.append(_rel(got, want))
        name = f"llm_logits/{wtype}_{mix}"
        record_observed(name, max(errs))
        assert max(errs) <= observed_bar(name, 3e-3 if wtype == "f16" else LOGIT_TOL), (max(errs), errs)
        assert decided >= 20 and len(set(ids)) >= 12, (decided, ids)   # the identical-ids statement above is about decisive, varied choices
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_f16_prompt_pass_of_600_rows_fused_launches(gpu_lib, tiny_files, tmpdir_models, monkeypatch):
    """Unquantised weights at prompt sizes (>= 512 rows: BASELINE configs[4]'s path) on a one-layer 2048-wide model with 16 heads of 128: the round-3 launches -- the 8-wave
    prompt attention storing fp16 rows for wo, w1|w3 with silu * mul in the epilogue, split-K combines
    folded into the next norm -- against (a) the same pass with MINIGPT4_F16_PAIR=0 / ATTN_PREFILL_W8=0 / DEFER_COMBINE=0 (separate launches): logits bit-identical, also after
    three more single-token steps that read the K / V rows the epilogue wrote; (b) the CPU oracle within the f16 tolerance."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    vp, _ = tiny_files
    lp = os.path.join(tmpdir_models, "llm_f16_2048x1.bin")
    if not os.path.exists(lp):
        G.write_llm_file(lp, G.tiny_llm(wtype="f16", n_embd=2048, n_layer=1, n_head=16, n_vocab=512), seed=3, std=0.02, **G.TINY_CONDITIONED)
    toks = [1] + [int(x) for x in np.random.default_rng(5).integers(3, 512, 599)]
    res = {}
    # "product": no switches at all -- since round 6 the pair epilogue COMPUTES the SiLU table's values (one fp16 ulp from the table in ~1e-4 of the values), so the launch-structure
    # identity below is checked with that one switch off in both arms (the separate launches gather from the table), and the product form is held to the oracle tolerance
    for mode in ("fused", "separate", "product"):
        for k in ("MINIGPT4_F16_PAIR", "MINIGPT4_ATTN_PREFILL_W8", "MINIGPT4_DEFER_COMBINE"):
            if mode == "product":
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, ("7" if k == "MINIGPT4_F16_PAIR" else "1") if mode == "fused" else "0")
        if mode == "product":
            monkeypatch.delenv("MINIGPT4_PAIR_SILU_COMPUTED", raising=False)
        else:
            monkeypatch.setenv("MINIGPT4_PAIR_SILU_COMPUTED", "0")
        ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=1024, n_batch=1024)
        try:
            gpu_lib.amd_eval_tokens(ctx, toks)
            a = gpu_lib.amd_logits(ctx)
            for t in (7, 300, 41):
                gpu_lib.amd_eval_tokens(ctx, [t])
            res[mode] = (a, gpu_lib.amd_logits(ctx))
        finally:
            gpu_lib.minigpt4_free(ctx)
    for i in range(2):
        assert np.array_equal(res["fused"][i].view(np.uint32), res["separate"][i].view(np.uint32)), (i, float(np.abs(res["fused"][i] - res["separate"][i]).max()))
    o = R.OracleLLM(G.read_llm_file(lp), n_ctx=1024)
    want = o.eval_tokens(toks)
    assert _rel(res["fused"][0], want) < 3e-3, _rel(res["fused"][0], want)
    assert _rel(res["product"][0], want) < 3e-3, _rel(res["product"][0], want)
    for t in (7, 300, 41):
        want = o.eval_tokens([t])
    assert _rel(res["fused"][1], want) < 3e-3, _rel(res["fused"][1], want)
    assert _rel(res["product"][1], want) < 3e-3, _rel(res["product"][1], want)


def test_fast_path_on_an_unconditioned_model_stays_within_the_oracles_own_noise(gpu_lib, tmpdir_models):
    """Whole-model check of the FAST kernels on plain i.i.d. Gaussian weights (no conditioning: no scaled residual writers, no output tie that would let the embedding term
    dominate the logits -- round-3 advisor finding).  Six layers, Q5_K_M mix; 24 embedding rows as the prompt, then 16 teacher-forced decode steps.  Criterion relative to what
    the arithmetic itself does: the oracle against ITSELF with the prompt rows perturbed by 3e-6 relative (every activation row is re-rounded to int8 before every mat-mul, so
    any change of summation order eventually flips a rounding) -- the GPU's mean |delta logit| must stay within 3x the run's largest self-noise (floor 5e-3 = one flipped
    rounding on a model this small) and under 2e-2 of the range."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    vp = os.path.join(tmpdir_models, "vision_tiny_iid.bin")
    if not os.path.exists(vp):
        G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=3, std=0.05)
    lp = os.path.join(tmpdir_models, "llm_iid_6l.bin")
    G.write_llm_file(lp, G.tiny_llm(wtype="q5_k", n_embd=256, n_layer=6, n_head=4, n_vocab=512, mix="q5_k_m"), seed=9, std=0.05)
    f = G.read_llm_file(lp)
    emb = (0.05 * np.random.default_rng(4).standard_normal((24, 256))).astype(np.float32)
    o, o2 = R.OracleLLM(f, n_ctx=64), R.OracleLLM(f, n_ctx=64)
    want, noisy = [o.eval_embd(emb)], [o2.eval_embd(emb * np.float32(1.0 + 3e-6))]
    ids = []
    for _ in range(16):
        ids.append(int(want[-1].argmax()))
        want.append(o.eval_tokens([ids[-1]])); noisy.append(o2.eval_tokens([ids[-1]]))
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=64, n_batch=32)
    try:
        gpu_lib.amd_eval_embd(ctx, emb)
        got = [gpu_lib.amd_logits(ctx).copy()]
        for t in ids:
            gpu_lib.amd_eval_tokens(ctx, [t])
            got.append(gpu_lib.amd_logits(ctx).copy())
    finally:
        gpu_lib.minigpt4_free(ctx)
    errs, noises = [], []
    for g, w, n in zip(got, want, noisy):
        rng_ = float(w.max() - w.min())
        errs.append(float(np.abs(g - w).mean()) / rng_); noises.append(float(np.abs(n - w).mean()) / rng_)
    # a step whose roundings the perturbation happened not to flip has zero self-noise, so the bar is the run's largest self-noise (floor: one flipped int8 rounding, 5e-3 of
    # the range on a model this small -- tests/conftest.py::observed_bar uses the same floor)
    bar = max(3.0 * max(noises), 5e-3)
    assert max(errs) <= bar and max(errs) < 2e-2, (errs, noises)
    from conftest import record_observed
    record_observed("iid_6l_q5_k_m_mean_abs_err_of_range", max(errs))


def test_eval_embd_matches_oracle(gpu_lib, tiny_files):
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m")
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=16)
    try:
        o = R.OracleLLM(G.read_llm_file(lp), n_ctx=96)
        emb = (0.05 * np.random.default_rng(3).standard_normal((32, 256))).astype(np.float32)
        gpu_lib.amd_eval_tokens(ctx, [1, 7, 9])
        o.eval_tokens([1, 7, 9])
        gpu_lib.amd_eval_embd(ctx, emb)
        want = o.eval_embd(emb)
        assert _rel(gpu_lib.amd_logits(ctx), want) < 2e-3
        assert gpu_lib.library.minigpt4_amd_n_past(ctx.ptr) == 35
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("n_batch,rows", [(16, 1), (32, 33), (8, 1)])
def test_single_embedding_row_chunk(gpu_lib, tiny_files, n_batch, rows):
    """A chunk that is exactly ONE embedding row (a 1-row llama_eval_embd, or pending rows == 1 mod n_batch ending in an embedding row) must read the
    embedding, not the previous decode token (round-1 advisor finding: forward(1) used to gather the stale d_feed token over it)."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m")
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=n_batch)
    try:
        o = R.OracleLLM(G.read_llm_file(lp), n_ctx=96)
        emb = (0.05 * np.random.default_rng(30 + rows).standard_normal((rows, 256))).astype(np.float32)
        gpu_lib.amd_eval_tokens(ctx, [1, 7, 9])
        o.eval_tokens([1, 7, 9])
        _ = gpu_lib.amd_logits(ctx)                   # forces the evaluation: the decode-token slot now holds a stale greedy id
        if n_batch == 8:                              # also leave a real decode step behind (d_feed = its token)
            gpu_lib.amd_eval_tokens(ctx, [11]); o.eval_tokens([11]); _ = gpu_lib.amd_logits(ctx)
        gpu_lib.amd_eval_embd(ctx, emb)
        want = o.eval_embd(emb)
        assert _rel(gpu_lib.amd_logits(ctx), want) < 2e-3
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_chat_flow_with_image_end_to_end(gpu_lib, tmpdir_models):
    """Reference call sequence (examples/main.cpp:207-293): load -> encode_image -> system_prompt -> begin_chat_image -> end_chat_image x K,
    on a model whose LLM width (4096) the C API accepts for image embeddings; greedy pieces identical to the oracle."""
    import refcpu as R
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G
    vp = os.path.join(tmpdir_models, "vision_e2e.bin")
    lp = os.path.join(tmpdir_models, "llm_e2e.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=11, std=0.05)
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=4096, n_layer=1, n_head=32, n_vocab=512, output_type="q6_k"), seed=2, std=0.02)
    bot = ML.MiniGPT4ChatBot(vp, lp, library=gpu_lib, n_ctx=256, n_batch=64)
    try:
        img = G.synth_image(42)
        bot.upload_image(img)                         # reset_chat + system_prompt + encode_image
        got = [t for _, t in zip(range(12), bot.generate("what is the text in the picture?", limit=12, temp=0.0, ignore_eos=True))]
        chat = R.OracleChat(R.OracleLLM(G.read_llm_file(lp), n_ctx=256), n_batch=64)
        chat.system_prompt()
        emb = R.OracleVision(G.read_vision_file(vp)).encode(img)
        chat.begin_chat_image(emb, b"what is the text in the picture?")
        want = [chat.end_chat(temp=0.0)[1].decode("utf-8", errors="replace") for _ in range(12)]
        assert got == want
        # follow-up turn without an image (begin_chat path)
        got2 = [t for _, t in zip(range(4), bot.generate("and now?", limit=4, temp=0.0, ignore_eos=True))]
        chat.begin_chat(b"and now?")
        want2 = [chat.end_chat(temp=0.0)[1].decode("utf-8", errors="replace") for _ in range(4)]
        assert got2 == want2
    finally:
        bot.free()


def test_odd_vocabulary_kquant_fallback_chat_flow(gpu_lib, tmpdir_models):
    """The type mix of the file a user of the reference really loads (ggml-vicuna-13B-v0-q5_k.bin, /root/reference/README.md:134): Vicuna-v0's n_vocab is 32001, not a
    multiple of 256, so llama.cpp's k-quant mixes leave output.weight in F16 and tok_embeddings in Q4_0 (modelgen.llm_tensor_types).  Here at tiny size with an ODD vocabulary
    (513: ragged last argmax partition, an F16 mat-vec with an odd row count, Q4_0 embedding rows) through the whole reference call sequence: greedy pieces identical and
    logits within 1e-2 in fast mode, logits bit-identical in parity mode."""
    import refcpu as R
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G, quants as Q
    vp = os.path.join(tmpdir_models, "vision_oddv.bin")
    lp = os.path.join(tmpdir_models, "llm_oddv.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=11, std=0.05)
    cfg = G.tiny_llm(wtype="q5_k", n_embd=4096, n_layer=2, n_head=32, n_vocab=513, mix="q5_k_m")
    types = G.llm_tensor_types(cfg)
    assert types["output.weight"] == Q.GGML_F16 and types["tok_embeddings.weight"] == Q.GGML_Q4_0 and types["layers.0.attention.wq.weight"] == Q.GGML_Q5_K
    G.write_llm_file(lp, cfg, seed=2, std=0.02, **G.TINY_CONDITIONED)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=256, n_batch=64)
    try:
        img = G.synth_image(42)
        emb = gpu_lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(img))
        emb_np = np.ctypeslib.as_array(emb.data, shape=(emb.n_embeddings,)).copy().reshape(32, -1)
        for parity in (False, True):
            gpu_lib.amd_set_parity(ctx, parity)
            gpu_lib.minigpt4_reset_chat(ctx)
            chat = R.OracleChat(R.OracleLLM(G.read_llm_file(lp), n_ctx=256), n_batch=64)
            gpu_lib.minigpt4_system_prompt(ctx)
            chat.system_prompt()
            gpu_lib.minigpt4_begin_chat_image(ctx, emb, "what is the text in the picture?")
            chat.begin_chat_image(emb_np, b"what is the text in the picture?")
            ids = []
            for step in range(16):
                got, want = gpu_lib.amd_logits(ctx), chat.llm.logits
                assert got.shape == (513,)
                if parity:
                    assert np.array_equal(got, want), (step, float(np.abs(got - want).max()))
                else:
                    assert _rel(got, want) <= LOGIT_TOL, (step, _rel(got, want))
                piece = gpu_lib.minigpt4_end_chat_image(ctx, temp=0.0)
                tid, opiece = chat.end_chat(temp=0.0)
                assert piece == opiece.decode("utf-8", errors="replace"), (parity, step)
                ids.append(int(tid))
            assert len(set(ids)) >= 6, ids
        gpu_lib.amd_set_parity(ctx, False)
        gpu_lib.minigpt4_free_embedding(emb)
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_decode_loop_device_feedback_equals_api_path(gpu_lib, tiny_files):
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m")
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=128, n_batch=16)
    try:
        gpu_lib.minigpt4_system_prompt(ctx)
        n0 = gpu_lib.library.minigpt4_amd_n_past(ctx.ptr)
        toks, ms = gpu_lib.amd_decode_loop(ctx, 16)
        assert ms > 0 and gpu_lib.library.minigpt4_amd_n_past(ctx.ptr) == n0 + 16
        gpu_lib.minigpt4_reset_chat(ctx)
        gpu_lib.minigpt4_system_prompt(ctx)
        ids = []
        tid = np.zeros(1, np.int32)
        for _ in range(16):
            assert gpu_lib.library.minigpt4_amd_sample(ctx.ptr, tid.ctypes.data_as(ML_INT_PTR()), 0.0, 40, 0.9, 1.0, 1.0, 0, 5.0, 1.0) == 0
            ids.append(int(tid[0]))
            gpu_lib.amd_eval_tokens(ctx, [int(tid[0])])
        assert ids == [int(t) for t in toks]
        prof = gpu_lib.amd_profile_sites(ctx, 2)                   # the eager launch set with a hipEvent pair per site: same tokens as the graph, a kernel symbol per site
        sites = {r["site"] for r in prof["sites"]}
        assert {"embed", "attention", "wo", "w2", "output", "argmax"} <= sites and all(r["avg_us"] > 0 and r["kernel"] for r in prof["sites"])
        assert any(r["site"] in ("qkv", "qk") for r in prof["sites"]) and prof["eager_ms_per_step"] > 0
    finally:
        gpu_lib.minigpt4_free(ctx)


def ML_INT_PTR():
    import ctypes
    return ctypes.POINTER(ctypes.c_int32)


def test_context_overflow_is_reported_not_fatal(gpu_lib, tiny_files):
    vp, llm = tiny_files
    ctx = gpu_lib.minigpt4_model_load(vp, llm("q4_0"), verbosity=0, n_ctx=16, n_batch=8)
    try:
        with pytest.raises(RuntimeError):
            gpu_lib.amd_eval_tokens(ctx, list(range(3, 23)))   # 20 tokens > n_ctx 16 -> FailedToAddString (reference would assert inside llama.cpp)
        assert gpu_lib.library.minigpt4_amd_n_past(ctx.ptr) == 0
        gpu_lib.amd_eval_tokens(ctx, [1, 2, 3])
        assert gpu_lib.library.minigpt4_amd_n_past(ctx.ptr) == 3
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("wtype,rows,cols", [("q5_k", 5120, 13824), ("q6_k", 32000, 5120), ("q4_0", 4096, 11008), ("f16", 32001, 5120), ("q8_0", 4096, 11008)])
def test_full_size_matvec_properties(gpu_lib, wtype, rows, cols):
    """BASELINE-size mat-vecs (13B w2, 13B output matrix, 7B w2): sampled rows against the oracle, plus size-independent properties --
    exact linearity in a power-of-two scaling of the weights' block scales, and row-permutation consistency."""
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    rng = np.random.default_rng(rows + cols)
    pool = (0.02 * rng.standard_normal(1 << 22)).astype(np.float32)
    w = np.resize(pool, rows * cols)
    raw = Q.quantize(t, w)
    x = rng.standard_normal((1, cols)).astype(np.float32)
    got = gpu_lib.amd_test_mul_mat(t, raw, cols, rows, x)[0]
    assert np.isfinite(got).all()
    rb = Q.nbytes(t, cols)
    pick = rng.choice(rows, 96, replace=False)
    sub = np.concatenate([raw[r * rb:(r + 1) * rb] for r in pick])
    want = R.mul_mat(t, sub, cols, len(pick), x)[0]
    assert np.abs(got[pick] - want).max() <= 2e-5 * np.abs(want).max()
    # the same rows in a different order give the same values (no cross-row state)
    perm = rng.permutation(rows)[:4096]
    raw_p = np.concatenate([raw[r * rb:(r + 1) * rb] for r in perm])
    got_p = gpu_lib.amd_test_mul_mat(t, raw_p, cols, len(perm), x)[0]
    assert np.array_equal(got_p, got[perm])
    # a checksum of the output equals the dot of the column-summed dequantised weights with the dequantised activations (fp64), loosely
    assert abs(float(got.astype(np.float64).sum())) < 1e6


@pytest.mark.parametrize("wtype,rows,cols", [("f16", 32001, 5120), ("q8_0", 4096, 11008)])
def test_full_size_narrow_unit_matvec_on_the_pipelined_kernel(gpu_lib, wtype, rows, cols):
    """The real Vicuna-v0 output matrix (F16, 32001 x 5120: an ODD row count over the persistent waves) and the 7B Q8_0 w2 (11 units per lane) through the decode path's own
    launch (k_matvec_v2 with the rms-norm prologue): sampled rows against the oracle on the identically prepared row, every row finite, and the launch's result equal to
    the generic tile kernel's (k_mul_mat: a different summation order) within fp32 noise on ALL rows."""
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    rng = np.random.default_rng(rows + cols)
    pool = (0.02 * rng.standard_normal(1 << 22)).astype(np.float32)
    raw = Q.quantize(t, np.resize(pool, rows * cols))
    x = rng.standard_normal(cols).astype(np.float32)
    nw = (1.0 + 0.2 * rng.standard_normal(cols)).astype(np.float32)
    got = gpu_lib.amd_test_matvec(t, raw, 1, cols, rows, x, nw, prep=1, fuse=True).reshape(-1)
    assert got.shape == (rows,) and np.isfinite(got).all()
    row = _prepared_row(1, x, nw, None)
    rb = Q.nbytes(t, cols)
    pick = np.concatenate([rng.choice(rows, 94, replace=False), [0, rows - 1]])
    sub = np.concatenate([raw[r * rb:(r + 1) * rb] for r in pick])
    want = R.mul_mat(t, sub, cols, len(pick), row[None, :])[0]
    assert np.abs(got[pick] - want).max() <= 2e-5 * np.abs(want).max()
    generic = gpu_lib.amd_test_mul_mat(t, raw, cols, rows, row[None, :])[0]
    assert np.abs(got - generic).max() <= 2e-5 * np.abs(generic).max()


def test_long_context_decode_matches_oracle(gpu_lib, tiny_files):
    """Attention over > 512 keys (several rounds of the key / value loops, KV cache far from empty), teacher-forced against the oracle."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    vp, llm = tiny_files
    lp = llm("q4_0", conditioned=True)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=1100, n_batch=512)
    try:
        o = R.OracleLLM(G.read_llm_file(lp), n_ctx=1100)
        rng = np.random.default_rng(4)
        toks = [1] + [int(t) for t in rng.integers(3, 512, 1040)]
        for i in range(0, len(toks), 512):
            gpu_lib.amd_eval_tokens(ctx, toks[i:i + 512])
            want = o.eval_tokens(toks[i:i + 512])
        got = gpu_lib.amd_logits(ctx)
        assert _rel(got, want) < LOGIT_TOL
        for _ in range(6):
            tid = int(want.argmax())
            gpu_lib.amd_eval_tokens(ctx, [tid])
            want = o.eval_tokens([tid])
            assert _rel(gpu_lib.amd_logits(ctx), want) < LOGIT_TOL
        assert gpu_lib.library.minigpt4_amd_n_past(ctx.ptr) == 1047
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_prompt_pass_beyond_the_prompt_attention_kernels_lds_rows(gpu_lib, tiny_files):
    """The prompt attention kernels keep 16 score rows of the WHOLE context in LDS: at this file's head size 64 they serve contexts up to 2240 keys (1984 at head size 128).  A prompt
    chunk that ends beyond that is routed through the decode attention kernel, one query row per workgroup (launch_attn_prefill returns false, Engine::forward falls back) --
    the logits must still be the oracle's, and decoding goes on from there."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    vp, llm = tiny_files
    lp = llm("q4_0", conditioned=True)
    f = G.read_llm_file(lp)
    assert f.hparams["n_embd"] // f.hparams["n_head"] == 64
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=2816, n_batch=512)
    try:
        o = R.OracleLLM(f, n_ctx=2816)
        rng = np.random.default_rng(9)
        toks = [1] + [int(t) for t in rng.integers(3, 512, 2700)]
        for i in range(0, len(toks), 512):                      # the chunks that end at 2560 and 2701 keys lie beyond every prompt kernel's range
            gpu_lib.amd_eval_tokens(ctx, toks[i:i + 512])
            want = o.eval_tokens(toks[i:i + 512])
            assert _rel(gpu_lib.amd_logits(ctx), want) < LOGIT_TOL, i
        for _ in range(3):
            tid = int(want.argmax())
            gpu_lib.amd_eval_tokens(ctx, [tid])
            want = o.eval_tokens([tid])
            assert _rel(gpu_lib.amd_logits(ctx), want) < LOGIT_TOL
        assert gpu_lib.library.minigpt4_amd_n_past(ctx.ptr) == 2704
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_batched_encode_images_equals_single(gpu_lib, tiny_files):
    import ctypes
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G
    vp, llm = tiny_files
    ctx = gpu_lib.minigpt4_model_load(vp, llm("q4_0"), verbosity=0, n_ctx=64, n_batch=32)
    try:
        # 10 images = one pass of 8 + one of 2 over the vision weights (Engine::VISION_BATCH_MAX); every image must equal its single-image encode bit for bit
        imgs = [G.synth_image(s) for s in range(1, 11)]
        structs = (ML.MiniGPT4Image * 10)(*[ML.array_to_image_struct(i) for i in imgs])
        batch = ML.MiniGPT4Images(structs, 10)
        out = ML.MiniGPT4Embeddings()
        assert gpu_lib.library.minigpt4_encode_images(ctx.ptr, ctypes.byref(batch), ctypes.byref(out), 0) == 0
        assert out.n_embeddings == 10
        for i, img in enumerate(imgs):
            single = gpu_lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(img))
            a = np.ctypeslib.as_array(single.data, shape=(single.n_embeddings,)).copy()
            b = np.ctypeslib.as_array(out.embeddings[i].data, shape=(out.embeddings[i].n_embeddings,)).copy()
            assert np.array_equal(a, b)
            gpu_lib.minigpt4_free_embedding(single)
        assert gpu_lib.library.minigpt4_free_embeddings(ctypes.byref(out)) == 0
        structs[1].format = 2                                                   # one U8 image in the batch: refused before any work (ImageNotF32)
        assert gpu_lib.library.minigpt4_encode_images(ctx.ptr, ctypes.byref(batch), ctypes.byref(out), 0) == 14 and not out.embeddings
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_temperature_sampling_path_runs_and_is_seeded(gpu_lib, tiny_files):
    """temp > 0: logits come back to the host sampler (top-k -> tfs -> typical -> top-p -> temp -> multinomial, mt19937(seed))."""
    vp, llm = tiny_files
    outs = []
    for _ in range(2):
        ctx = gpu_lib.minigpt4_model_load(vp, llm("q4_0"), verbosity=0, seed=99, n_ctx=96, n_batch=32)
        try:
            gpu_lib.minigpt4_begin_chat(ctx, "hello")
            outs.append([gpu_lib.minigpt4_end_chat(ctx, temp=0.8, top_k=40, top_p=0.9) for _ in range(8)])
        finally:
            gpu_lib.minigpt4_free(ctx)
    assert outs[0] == outs[1]


def test_key_split_attention_at_the_13b_head_count_is_bit_identical(gpu_lib):
    """The key-split decode attention at the REAL head count (40 heads x 6 splits = 240 workgroups over all 8 XCDs; 13B width, two layers): its last-arriver combine reads the
    other workgroups' partial sums through write-through stores + drained arrival + sc1 loads (k_attn_split_pv, cdna_hip_programming.md Guideline 16 R1).  A stale partial
    would show as run-to-run differences or as a large error: the same 48 steps at 800+ cached keys twice in one context must give bit-identical logits, the same greedy ids as
    the one-workgroup-per-head kernel (MINIGPT4_ATTN_SPLIT_T=0), and logits within 1e-2 of it (the P.V partial sums are added in another order)."""
    import headline as H
    vp, lp = H.headline_files("13b_l2")
    rng = np.random.default_rng(23)
    toks = [1] + [int(t) for t in rng.integers(3, 31000, 811)]
    runs = {}
    for thr in (None, "0"):
        if thr is not None:
            os.environ["MINIGPT4_ATTN_SPLIT_T"] = thr
        try:
            ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=1024, n_batch=512)
        finally:
            os.environ.pop("MINIGPT4_ATTN_SPLIT_T", None)
        try:
            passes = []
            for _ in range(2 if thr is None else 1):
                gpu_lib.minigpt4_reset_chat(ctx)
                gpu_lib.amd_eval_tokens(ctx, toks)
                got = gpu_lib.amd_logits(ctx)
                ids, lg = [], []
                for step in range(48):
                    tid = int(got.argmax()); ids.append(tid)
                    gpu_lib.amd_eval_tokens(ctx, [tid])
                    got = gpu_lib.amd_logits(ctx).copy()
                    lg.append(got)
                passes.append((ids, lg))
            runs[thr] = passes
        finally:
            gpu_lib.minigpt4_free(ctx)
    (ids_a, lg_a), (ids_b, lg_b) = runs[None]
    assert ids_a == ids_b
    for i, (a, b) in enumerate(zip(lg_a, lg_b)):
        assert np.isfinite(a).all() and np.array_equal(a, b), (i, float(np.abs(a - b).max()))
    ids_0, lg_0 = runs["0"][0]
    assert ids_a == ids_0
    for a, b in zip(lg_a, lg_0):
        assert _rel(a, b) < 1e-2


@pytest.mark.parametrize("n_embd,n_head", [(256, 4), (512, 4), (128, 4)])      # head sizes 64, 128, 32
def test_key_split_decode_attention_matches_the_single_workgroup_kernel_and_the_oracle(gpu_lib, tmpdir_models, n_embd, n_head):
    """Long contexts: the decode step shares every head's keys between workgroups (k_attn_split_scores / k_attn_split_pv, two launches, last-arriver combine).  Same
    conversation evaluated with the split attention from 48 cached keys on (MINIGPT4_ATTN_SPLIT_T=48: the captured step is re-captured when the context crosses it) and with
    the one-workgroup-per-head kernel only (=0): logits equal up to the fp32 order of the P.V partial sums, greedy ids identical, and both within 1e-2 of the CPU oracle."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    vp = os.path.join(tmpdir_models, "vision_tiny_split.bin")
    if not os.path.exists(vp):
        G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=3, std=0.05)
    lp = os.path.join(tmpdir_models, f"llm_split_{n_embd}.bin")
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=n_embd, n_layer=2, n_head=n_head, n_vocab=512), seed=5, std=0.05, **G.TINY_CONDITIONED)
    rng = np.random.default_rng(11)
    toks = [1] + [int(t) for t in rng.integers(3, 512, 39)]       # 40 prompt rows, then 700 decode steps: the context crosses 48 and grows to 740
    o = R.OracleLLM(G.read_llm_file(lp), n_ctx=768)
    want = o.eval_tokens(toks)
    runs = {}
    for thr in ("48", "0"):
        os.environ["MINIGPT4_ATTN_SPLIT_T"] = thr
        try:
            ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=768, n_batch=64)
        finally:
            os.environ.pop("MINIGPT4_ATTN_SPLIT_T", None)
        try:
            gpu_lib.amd_eval_tokens(ctx, toks)
            got = gpu_lib.amd_logits(ctx)
            ids, lg = [], [got.copy()]
            for step in range(700):
                tid = int(got.argmax())
                ids.append(tid)
                gpu_lib.amd_eval_tokens(ctx, [tid])
                got = gpu_lib.amd_logits(ctx)
                if step % 50 == 49 or step < 12:
                    lg.append(got.copy())
            runs[thr] = (ids, lg)
        finally:
            gpu_lib.minigpt4_free(ctx)
    assert runs["48"][0] == runs["0"][0]
    for a, b in zip(runs["48"][1], runs["0"][1]):
        assert _rel(a, b) < 1e-2
    ow = want
    for step, tid in enumerate(runs["48"][0][:60]):               # the oracle along the same greedy path
        assert int(ow.argmax()) == tid, step
        ow = o.eval_tokens([tid])


@pytest.mark.parametrize("shape", [(32, 768, 768), (32, 768, 2304), (32, 3072, 768), (32, 768, 3072), (32, 768, 5120), (64, 768, 768), (96, 768, 2304), (256, 3072, 768), (1, 64, 16),
                                   (33, 96, 48), (17, 768, 4096)])
@pytest.mark.parametrize("gelu", [False, True])
def test_gemm_f16_skinny_kernel(gpu_lib, shape, gelu):
    """k_gemm_f16_skinny (the Q-Former's GEMMs: few rows, N / 16 workgroups, K split across the four waves) against a float64 product of the fp16-rounded operands, and
    against the 64x64-tile kernel (same exact products, another fp32 order)."""
    import refcpu as R
    M, K, N = shape
    rng = np.random.default_rng(M * 11 + K + N)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (0.1 * rng.standard_normal((N, K))).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    got = gpu_lib.amd_test_gemm_f16(A, W, b, gelu, skinny=True)
    ref = A.astype(np.float16).astype(np.float64) @ W.astype(np.float16).astype(np.float64).T + b
    if gelu:
        tab = R.table(0).view(np.float16)
        ref32 = (A.astype(np.float16).astype(np.float64) @ W.astype(np.float16).astype(np.float64).T).astype(np.float32) + b
        want = tab[ref32.astype(np.float16).view(np.uint16)].astype(np.float32)
        assert (np.abs(got - want) > 2e-3 * (1 + np.abs(want))).mean() < 2e-3
    else:
        assert _rel(got, ref) < 2e-5
        assert _rel(got, gpu_lib.amd_test_gemm_f16(A, W, b, gelu)) < 2e-5


def test_round6_encoder_arms_are_bit_identical_at_full_size(gpu_lib, monkeypatch):
    """Round-6 changes of the image path that must not change a bit, at the real ViT-g/14 shapes (1408 wide, 16 heads of 88, 257 rows per image; 39 blocks sharing one set
    of weights): (1) the split-K GEMM's work list dealt to the XCDs by K slice (MINIGPT4_SPLITK_XCD=0: slices in grid.z as in rounds 3-5); (2) fc2 of several images on the
    LDS-DMA ring tiles (128x128 at two images, 256x128 from three) -- same K slice boundaries, so image b of a batch still equals the image encoded alone; (3) the looping
    form of the vision attention (MINIGPT4_ATTN_QT=2 / 5 query tiles per workgroup) against the single-tile kernel; (4) the Q-Former's split-K dense layers against the
    whole-K form (close, not identical).  One image, a batch of two and a batch of three per arm."""
    import headline as H
    from minigpt4_cpp_amd import modelgen as G
    vp, _ = H.headline_files("13b_l2")
    lp = os.path.join(H.model_dir(), "llm_tiny_for_vision.bin")
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=256, n_layer=1, n_head=4, n_vocab=512), seed=2, std=0.05)
    imgs = [G.synth_image(60 + i) for i in range(3)]

    def run(env):
        for k in ("MINIGPT4_SPLITK_XCD", "MINIGPT4_ATTN_QT", "MINIGPT4_QF_FOLD", "MINIGPT4_KV_HOIST", "MINIGPT4_QF_SPLITK", "MINIGPT4_QKV_HEAD_MAJOR"):   # each read per context, at load: an arm sets only what it names
            if k in env:
                monkeypatch.setenv(k, env[k])
            else:
                monkeypatch.delenv(k, raising=False)
        ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=64, n_batch=32)
        try:
            one = gpu_lib.amd_encode_images(ctx, imgs[:1])[0]
            two = gpu_lib.amd_encode_images(ctx, imgs[:2])
            three = gpu_lib.amd_encode_images(ctx, imgs)
            return one, two, three
        finally:
            gpu_lib.minigpt4_free(ctx)

    base1, base2, base3 = run({})
    assert np.isfinite(base1).all() and np.abs(base1).max() > 0
    assert np.array_equal(base3[0], base1) and np.array_equal(base2[0], base1) and np.array_equal(base2[1], base3[1])   # batched = alone, across the three fc2 tile shapes
    assert not np.array_equal(base3[1], base3[0])
    try:
        # (round 5's two Q-Former arms ride along: the constant head of layer 0 recomputed per encode, one K | V projection per cross layer -- same launches, same bits)
        for env in ({"MINIGPT4_SPLITK_XCD": "0"}, {"MINIGPT4_ATTN_QT": "2"}, {"MINIGPT4_ATTN_QT": "5"}, {"MINIGPT4_QF_FOLD": "0"}, {"MINIGPT4_KV_HOIST": "0"},
                    {"MINIGPT4_QKV_HEAD_MAJOR": "0"}):                     # q | k | v as rows of 3 x D instead of [3][head][rows][88]: only addresses differ
            one, two, three = run(env)
            assert np.array_equal(one, base1), env
            assert all(np.array_equal(a, b) for a, b in zip(three, base3)) and all(np.array_equal(a, b) for a, b in zip(two, base2)), env
        # (4) the Q-Former's dense / output layers with K split over 2 / 4 workgroups + LayerNorm in the slab reduce: another fp32 summation order of the same products
        # -- not bit-identical to the whole-K form, but as close to it as two orders of 768 .. 3072 fp32 terms are, and batched = alone in both forms
        one, two, three = run({"MINIGPT4_QF_SPLITK": "0"})
        assert np.array_equal(three[0], one) and np.array_equal(two[1], three[1])
        d = float(np.abs(one - base1).max() / np.abs(base1).max())
        print(f"Q-Former split-K vs whole-K dense layers: max rel diff of the embedding {d:.2e}")
        # (observed 5.4e-4 of the largest element: a different fp32 order flips a few fp16 roundings of the LayerNorm outputs, and twelve layers carry them on -- the size of
        # fast mode's own distance to the oracle, which test_full_size_vit_g_encode_matches_oracle bounds for the form that ships)
        assert 0.0 < d < 2e-3, d
    finally:
        run({})                                                          # leave the process-wide switches at their defaults


@pytest.mark.parametrize("arm", ["0", "1"])
def test_table_gather_and_computed_table_arms_match_the_oracle(gpu_lib, tiny_files, monkeypatch, arm):
    """MINIGPT4_COMPUTED_TABLES (round-5 advisor: the deviation must be stated and the other arm kept under test).  "1" (default): fast mode's decode step and the ViT / Q-Former
    attention COMPUTE the values of ggml's fp16 exp / SiLU tables (fp16(f(fp16 x)) with the device's exp: equal to the host table's entry except within ~1e-7 of an fp16 rounding
    boundary); "0": they gather from the tables as ggml does.  Both arms through the reference call sequence on a conditioned model: image embedding within the vision bar of the
    oracle, greedy pieces identical to the oracle's, decode logits within north_star's 1e-2 of the largest |logit| (observed: a few 1e-3, the re-rounding noise of the model)."""
    import refcpu as R
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    monkeypatch.setenv("MINIGPT4_COMPUTED_TABLES", arm)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=256, n_batch=64)
    try:
        img = G.synth_image(5)
        emb = gpu_lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(img))
        got = np.ctypeslib.as_array(emb.data, shape=(emb.n_embeddings,)).copy().reshape(32, -1)
        gpu_lib.minigpt4_free_embedding(emb)
        want = R.OracleVision(G.read_vision_file(vp)).encode(img)
        assert float(np.abs(got - want).max() / np.abs(want).max()) < 3e-3
        chat = R.OracleChat(R.OracleLLM(G.read_llm_file(lp), n_ctx=256), n_batch=64)
        gpu_lib.minigpt4_system_prompt(ctx)
        chat.system_prompt()
        gpu_lib.minigpt4_begin_chat(ctx, "what is the text in the picture?")
        chat.begin_chat(b"what is the text in the picture?")
        worst = 0.0
        for _ in range(12):                                                 # every step after the first is a decode step (the arm's kernels)
            lg, ol = gpu_lib.amd_logits(ctx), chat.llm.logits
            worst = max(worst, float(np.abs(lg - ol).max() / np.abs(ol).max()))
            assert gpu_lib.minigpt4_end_chat(ctx, temp=0.0) == chat.end_chat(temp=0.0)[1].decode("utf-8", errors="replace")
        print(f"MINIGPT4_COMPUTED_TABLES={arm}: max logit rel {worst:.2e}")
        assert worst <= 1e-2, worst
    finally:
        gpu_lib.minigpt4_free(ctx)
