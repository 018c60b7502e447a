"""Q3_K streamed natively (3.4-bit planes: plan_qweight / k_repack; Tr<GT_Q3_K>; csrc/mmq2_q3k.hip), no Q6_K image.  Arbitrary block bytes of both generators of
tests/quant_blocks.py -- `extreme` has the all-zero block, scale -32 x weight -4, the one product that is an int8 byte only after negation -- against float64 under the
derived fp32 bound (ratio <= 1):
  1. k_mmq2_q3k<TT>: a partial tile and a single super-block; two tiles, two matrices, ragged rows; a forced K split with a residual; three token tiles x three matrices
     with a ragged 33rd weight row; an odd super-block count (K = 768);
  2. without a K split its outputs equal the oracle-order kernel's (k_mul_mat_ref) bit for bit;
  3. k_matvec_v2 (rows prepared by a launch of their own): 1, 3 (ragged), 6 (ragged) and 7 units per lane, one and three matrices of 130 rows;
  4. k_matvec_tn: 2, 3 and 4 rows at one and three units per lane;
  5. a tiny q3_k file through the C ABI: the engine streams the FILE's bytes per token, and a 37-row prompt pass, batched steps of 8 (k_mmq2_q3k) and of 3 conversations
     (k_matvec_tn) and 8 single decode steps stay within LOGIT_TOL of the CPU oracle."""
import ctypes

import numpy as np
import pytest
import quant_blocks as QB

pytestmark = pytest.mark.gpu
T = QB.Q3_K
MMQ2_SHAPES = QB.MMQ2_SHAPES + [(70, 512, 33, 3, 0, False), (33, 768, 70, 1, 0, False)]
gens = pytest.mark.parametrize("gen", ["random", "extreme"])


def _ratio(gen, n_rows_set, K, got, idx, rows, residual=None):
    exact, mag = QB.reference(gen, T, n_rows_set, K)
    assert got.shape == (len(idx), rows.stop - rows.start) and np.isfinite(got).all()
    return QB.ratio_of(got, exact[idx][:, rows], mag[idx][:, rows], QB.n_blocks(T, K), residual)


def _assert_all(what, ratios):
    print("q3k_native %s: worst ratio %.4f" % (what, max(ratios.values())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


@gens
@pytest.mark.parametrize("shape", MMQ2_SHAPES, ids=lambda c: "N%d_K%d_R%d_m%d_ks%d_res%d" % c)
def test_mmq2_q3k_on_arbitrary_blocks(gpu_lib, gen, shape):
    N, K, n_out, n_mat, ks, with_res = shape
    res = np.random.default_rng(N + K).integers(-3, 4, (n_mat, N, n_out)).astype(np.float32) if with_res else None
    got = gpu_lib.amd_test_mmq2(T, QB.blocks(gen, T, n_mat * n_out, K).reshape(-1), n_mat, K, n_out, QB.act_rows(T, K, N), residual=res, ks=ks, generation=2)
    _assert_all("mmq2 %s %s" % (gen, shape), {m: _ratio(gen, n_mat * n_out, K, got[m], QB.rows_index(N), slice(m * n_out, (m + 1) * n_out),
                                                         None if res is None else res[m].astype(np.float64)) for m in range(n_mat)})


@gens
def test_no_k_split_is_the_oracle_order_bit_for_bit(gpu_lib, gen):
    N, K, n_out = 33, 1024, 70
    raw, x = QB.blocks(gen, T, n_out, K).reshape(-1), QB.act_rows(T, K, N)
    got = gpu_lib.amd_test_mmq2(T, raw, 1, K, n_out, x, ks=1, generation=2)[0]
    want = gpu_lib.amd_test_mul_mat(T, raw, K, n_out, x, ref=True)
    assert np.array_equal(got, want), (int((got != want).sum()), float(np.abs(got - want).max()))


@gens
@pytest.mark.parametrize("n_mat", [1, 3])
@pytest.mark.parametrize("K", [512, 5120, 11008, 13824])
def test_decode_matvec_on_arbitrary_blocks(gpu_lib, gen, K, n_mat):
    rows = 130
    raw = QB.blocks(gen, T, 3 * rows, K)[:n_mat * rows]
    _assert_all("matvec %s K%d m%d" % (gen, K, n_mat), {
        a: _ratio(gen, 3 * rows, K, gpu_lib.amd_test_matvec(T, raw.reshape(-1), n_mat, K, rows, QB.activation_rows(T, K)[a], prep=2, fuse=False).reshape(1, n_mat * rows),
                  [a], slice(0, n_mat * rows)) for a in range(6)})


@gens
@pytest.mark.parametrize("n_mat", [1, 3])
@pytest.mark.parametrize("N", [2, 3, 4])
@pytest.mark.parametrize("K", [512, 5120])
def test_multi_row_matvec_on_arbitrary_blocks(gpu_lib, gen, K, N, n_mat):
    rows = 130
    raw = QB.blocks(gen, T, 3 * rows, K)[:n_mat * rows]
    ratios = {}
    for first in (0, 3):
        got = gpu_lib.amd_test_matvec_rows(T, raw.reshape(-1), n_mat, K, rows, QB.act_rows(T, K, N, first), prepare=False)
        ratios.update({(first, m): _ratio(gen, 3 * rows, K, got[m], QB.rows_index(N, first), slice(m * rows, (m + 1) * rows)) for m in range(n_mat)})
    _assert_all("matvec_rows %s K%d N%d m%d" % (gen, K, N, n_mat), ratios)


def test_tiny_q3k_file_streams_its_own_bytes_and_matches_the_oracle(gpu_lib, tiny_files):
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    from test_gpu_parity import LOGIT_TOL, _rel
    vp, llm = tiny_files
    lp = llm("q3_k", conditioned=True)
    f = G.read_llm_file(lp)
    file_bytes = ctypes.c_int64(0)
    assert gpu_lib.library.minigpt4_amd_inspect_files(None, lp.encode(), None, None, ctypes.byref(file_bytes)) == 0
    rng = np.random.default_rng(13)
    prompts = [[1] + [int(v) for v in rng.integers(3, 512, 36)]] + [[1] + [int(v) for v in rng.integers(3, 512, 2 + s)] for s in range(1, 8)]
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=96, n_batch=64)
    try:
        assert gpu_lib.library.minigpt4_amd_weight_bytes_per_token(ctx.ptr) == float(file_bytes.value)   # was 210 / 110 of it on the Q3_K tensors
        gpu_lib.amd_set_conversations(ctx, 8)
        oracles, errs = [R.OracleLLM(f, n_ctx=96) for _ in prompts], {}
        for s, (p, o) in enumerate(zip(prompts, oracles)):          # conversation 0: 37 rows, two token tiles of k_mmq2_q3k
            gpu_lib.amd_select_conversation(ctx, s)
            gpu_lib.amd_eval_tokens(ctx, p)
            errs["prompt", s] = _rel(gpu_lib.amd_logits(ctx), o.eval_tokens(p))
        for slots in (list(range(8)), [1, 4, 6]):                   # 8 rows: k_mmq2_q3k; 3 rows: k_matvec_tn
            nxt = [int(v) for v in rng.integers(3, 512, len(slots))]
            gpu_lib.amd_select_conversation(ctx, slots[0])
            gpu_lib.amd_eval_batch(ctx, slots, nxt)
            for s, t in zip(slots, nxt):
                gpu_lib.amd_select_conversation(ctx, s)
                errs["batch", len(slots), s] = _rel(gpu_lib.amd_logits(ctx), oracles[s].eval_tokens([t]))
        gpu_lib.amd_select_conversation(ctx, 0)
        for step in range(8):                                       # single decode steps: k_matvec_v2
            t = int(rng.integers(3, 512))
            gpu_lib.amd_eval_tokens(ctx, [t])
            errs["decode", step] = _rel(gpu_lib.amd_logits(ctx), oracles[0].eval_tokens([t]))
        print("q3k_native tiny file: worst logit error %.3e of the largest |logit|" % max(errs.values()))
        assert max(errs.values()) <= LOGIT_TOL, {k: v for k, v in errs.items() if v > LOGIT_TOL}
    finally:
        gpu_lib.minigpt4_free(ctx)
