"""The Q2_K member of the generation-2 prompt mat-mul family (csrc/mmq2_q2k.hip, k_mmq2_q2k<TT>: sub-block scale x quant as ONE int8 operand byte):
  1. arbitrary block bytes against float64 under the derived fp32 bound of tests/quant_blocks.py (ratio <= 1): its three MMQ2_SHAPES (one partial tile and a single super-block;
     two tiles, two matrices, ragged rows; a forced K split with a residual), three token tiles in one chunk with three matrices and a ragged 33rd weight row, and an odd
     super-block count (K = 768);
  2. without a K split the kernel's outputs equal the oracle-order kernel's (k_mul_mat_ref) bit for bit;
  3. a tiny q2_k file through the C ABI: a 37-row prompt pass and a batched step of 8 conversations against the CPU oracle, 1e-2 of the largest |logit|."""
import numpy as np
import pytest
import quant_blocks as QB

pytestmark = pytest.mark.gpu
SHAPES = QB.MMQ2_SHAPES + [(70, 512, 33, 3, 0, False), (33, 768, 70, 1, 0, False)]
gens = pytest.mark.parametrize("gen", ["random", "extreme"])


@gens
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "N%d_K%d_R%d_m%d_ks%d_res%d" % c)
def test_mmq2_q2k_on_arbitrary_blocks(gpu_lib, gen, shape):
    N, K, n_out, n_mat, ks, with_res = shape
    idx = QB.rows_index(N)
    res = np.random.default_rng(N + K).integers(-3, 4, (n_mat, N, n_out)).astype(np.float32) if with_res else None
    got = gpu_lib.amd_test_mmq2(QB.Q2_K, QB.blocks(gen, QB.Q2_K, n_mat * n_out, K).reshape(-1), n_mat, K, n_out, QB.act_rows(QB.Q2_K, K, N), residual=res, ks=ks, generation=2)
    exact, mag = QB.reference(gen, QB.Q2_K, n_mat * n_out, K)
    ratios = {}
    for m in range(n_mat):
        rows = slice(m * n_out, (m + 1) * n_out)
        assert got[m].shape == (N, n_out) and np.isfinite(got[m]).all(), m
        ratios[m] = QB.ratio_of(got[m], exact[idx][:, rows], mag[idx][:, rows], QB.n_blocks(QB.Q2_K, K), None if res is None else res[m].astype(np.float64))
        print("mmq2_q2k %s %s mat%d: ratio %.4f" % (gen, shape, m, ratios[m]))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


@gens
def test_no_k_split_is_the_oracle_order_bit_for_bit(gpu_lib, gen):
    N, K, n_out = 33, 1024, 70
    raw, x = QB.blocks(gen, QB.Q2_K, n_out, K).reshape(-1), QB.act_rows(QB.Q2_K, K, N)
    got = gpu_lib.amd_test_mmq2(QB.Q2_K, raw, 1, K, n_out, x, ks=1, generation=2)[0]
    want = gpu_lib.amd_test_mul_mat(QB.Q2_K, raw, K, n_out, x, ref=True)
    assert np.array_equal(got, want), (int((got != want).sum()), float(np.abs(got - want).max()))


def test_prompt_pass_and_batched_step_against_the_oracle(gpu_lib, tiny_files):
    """37 prompt rows (two token tiles) through amd_eval_tokens, then one amd_eval_batch step of 8 conversations (a few rows of one tile): every matrix of the q2_k file,
    its output matrix included, runs on k_mmq2_q2k"""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    from test_gpu_parity import LOGIT_TOL, _rel
    vp, llm = tiny_files
    lp = llm("q2_k", conditioned=True)
    f = G.read_llm_file(lp)
    rng = np.random.default_rng(11)
    prompts = [[1] + [int(v) for v in rng.integers(3, 512, 36)]] + [[1] + [int(v) for v in rng.integers(3, 512, 2 + s)] for s in range(1, 8)]
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=96, n_batch=64)
    try:
        gpu_lib.amd_set_conversations(ctx, 8)
        oracles, errs = [R.OracleLLM(f, n_ctx=96) for _ in prompts], []
        for s, (p, o) in enumerate(zip(prompts, oracles)):
            gpu_lib.amd_select_conversation(ctx, s)
            gpu_lib.amd_eval_tokens(ctx, p)
            errs.append(_rel(gpu_lib.amd_logits(ctx), o.eval_tokens(p)))
        assert max(errs) <= LOGIT_TOL, errs
        gpu_lib.amd_select_conversation(ctx, 0)
        nxt = [int(v) for v in rng.integers(3, 512, 8)]
        gpu_lib.amd_eval_batch(ctx, list(range(8)), nxt)
        errs = []
        for s, o in enumerate(oracles):
            gpu_lib.amd_select_conversation(ctx, s)
            errs.append(_rel(gpu_lib.amd_logits(ctx), o.eval_tokens([nxt[s]])))
        print("mmq2_q2k batched step of 8: worst logit error %.3e of the largest |logit|" % max(errs))
        assert max(errs) <= LOGIT_TOL, errs
    finally:
        gpu_lib.minigpt4_free(ctx)
