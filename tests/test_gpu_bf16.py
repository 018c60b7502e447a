"""BF16 weights (GGUF type 30) on the GPU against float64: weights widened exactly, rows rounded to bfloat16 in NumPy, dots in float64, under the fp32 accumulation
bound of tests/quant_blocks.py ((terms + 4) x 2^-24 x sum |w a|, one term per element; ratio <= 1).  Decode: k_matvec_v2_free at 1, 2 (K = 1032: masked tail in the
8-unit form) and 10 units per lane, K = 5128 and rows 2 .. 15 on k_mul_mat.  k_gemm_bf16: the launcher's own rule splits K (8 slices) for every K = 4104 case whose
N x n_out is a multiple of 4 and for no other case (K = 64 | 72: one or two steps; N = 17 | 33 with n_out = 130: the flat combine does not apply).  The embedding
gather bit for bit.  A tiny all-BF16 GGUF file against the CPU oracle on its F32 twin: prompt pass and 8 decode steps within LOGIT_TOL."""
import numpy as np
import pytest
import quant_blocks as QB

pytestmark = pytest.mark.gpu
BF16 = 30


def _case(N, K, n_out):
    from minigpt4_cpp_amd import quants as Q
    rng = np.random.default_rng([N, K, n_out])
    w = Q.quantize(BF16, rng.standard_normal(n_out * K).astype(np.float32) * np.float32(0.05)).view(np.uint16)
    x = rng.standard_normal((N, K)).astype(np.float32)
    return w, x, Q.dequantize_bf16(w).astype(np.float64).reshape(n_out, K), Q.dequantize_bf16(Q.quantize_bf16(x)).astype(np.float64).reshape(N, K)


def _check(what, got, w64, x64, residual=None):
    r = QB.ratio(got, x64, w64, np.abs(w64), x64.shape[1], residual)
    print("bf16 %s: error / bound %.4f" % (what, r))
    assert r <= 1.0


@pytest.mark.parametrize("N,K,n_out", [(1, K, R) for K in (512, 1024, 1032, 5120, 5128) for R in (33, 64)] + [(N, 1024, 33) for N in (2, 4, 5, 15)])
def test_decode_matvec_and_few_rows(gpu_lib, N, K, n_out):
    w, x, w64, x64 = _case(N, K, n_out)
    if N == 1 and K <= 5120:   # the pipelined kernel itself: the hook fails where launch_matvec_set refuses
        _check("matvec K%d R%d" % (K, n_out), gpu_lib.amd_test_matvec(BF16, w, 1, K, n_out, x[0], prep=2, fuse=False).reshape(1, n_out), w64, x64)
    _check("mul_mat N%d K%d R%d" % (N, K, n_out), gpu_lib.amd_test_mul_mat(BF16, w, K, n_out, x), w64, x64)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("n_out", [32, 130])
@pytest.mark.parametrize("K", [64, 72, 4104])
@pytest.mark.parametrize("N", [16, 17, 33, 160])
def test_gemm_bf16(gpu_lib, N, K, n_out, with_res):
    w, x, w64, x64 = _case(N, K, n_out)
    res = np.random.default_rng(N + K).integers(-3, 4, (1, N, n_out)).astype(np.float32) if with_res else None
    got = gpu_lib.amd_test_mmq2(BF16, w, 1, K, n_out, x, residual=res, ks=0)[0]
    _check("gemm N%d K%d R%d res%d" % (N, K, n_out, with_res), got, w64, x64, None if res is None else res[0].astype(np.float64))


def test_get_rows_bit_for_bit(gpu_lib):
    w, _, w64, _ = _case(1, 264, 37)
    tok = [0, 36, 5, 5]
    got = gpu_lib.amd_test_get_rows(BF16, w, 37, 264, tok).view(np.uint32)
    assert np.array_equal(got[:4], w64[tok].astype(np.float32).view(np.uint32)) and (got[4] == 0xFFFFFFFF).all()


def test_tiny_bf16_gguf_matches_the_oracle_on_its_f32_twin(gpu_lib, tiny_files, tmp_path):
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    from test_gpu_parity import LOGIT_TOL, _rel
    vp, llm = tiny_files
    src, gguf, twin = llm("bf16", conditioned=True), str(tmp_path / "bf16.gguf"), str(tmp_path / "f32_twin.bin")
    G.ggjt_to_gguf(src, gguf)
    G.write_q8_0_twin(src, twin)
    oracle = R.OracleLLM(G.read_llm_file(twin), n_ctx=96)
    rng = np.random.default_rng(17)
    prompt = [1] + [int(v) for v in rng.integers(3, 512, 36)]      # 37 rows: two token tiles of k_gemm_bf16
    ctx = gpu_lib.minigpt4_model_load(vp, gguf, verbosity=0, n_ctx=96, n_batch=64)
    try:
        gpu_lib.amd_eval_tokens(ctx, prompt)
        want = oracle.eval_tokens(prompt)
        errs = {"prompt": _rel(gpu_lib.amd_logits(ctx), want)}
        for step in range(8):                                       # fed the oracle's tokens: no free-running ids, no near-tie decides
            t = int(np.argmax(want))
            gpu_lib.amd_eval_tokens(ctx, [t])
            want = oracle.eval_tokens([t])
            errs["decode", step] = _rel(gpu_lib.amd_logits(ctx), want)
        print("bf16 tiny file: worst logit error %.3e of the largest |logit|" % max(errs.values()))
        assert max(errs.values()) <= LOGIT_TOL, errs
    finally:
        gpu_lib.minigpt4_free(ctx)
