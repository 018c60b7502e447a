"""GGUF IQ4_NL / IQ4_XS: the lookup mat-vec traits, the int8-MFMA prompt kernel k_mmq2_iq4, the embedding gather, and whole files through the C ABI.
Kernel cases: arbitrary block bytes against the float64 decoder BELOW (from the bit fields, not quants.dequantize_*), with the integer activation rows, the derived bound and
the shapes of tests/quant_blocks.py: |got - x . w| <= (n_blocks + 4) * 2^-24 * (|x| . |w|) per output (one-term forms: a = |w|).  Three fills, the sign of d alternating from
block to block: uniform random bytes; all 0x00 (code -127, ls - 32 = -32); all 0xFF (code 113, ls - 32 = 31).  A hook that refuses a shape raises, which fails the test.
End to end: the CPU oracle does not know these formats and evaluates the file's Q8_0 twin (quants.iq4_to_q8_0), exact for d_bits = 5 (tests/test_cpu_iq4.py)."""
import functools
import os

import numpy as np
import pytest
import quant_blocks as QB

pytestmark = pytest.mark.gpu
NL, XS, NAMES = 20, 23, {20: "iq4_nl", 23: "iq4_xs"}
BLOCK = {NL: (32, 18), XS: (256, 136)}
ACT = {NL: QB.Q4_0, XS: QB.Q4_K}                                  # whose activation rows (Q8_0 / Q8_K exact) the type multiplies
KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.float64)
FILLS = ("random", 0x00, 0xFF)
both = pytest.mark.parametrize("t", [NL, XS], ids=lambda t: NAMES[t])


def decode_iq4(t, raw, n):
    """float64 [n] from the block bytes.  IQ4_NL: fp16 d | qs[16].  IQ4_XS: fp16 d | u16 scales_h | scales_l[4] | qs[128], sub-block ib = qs[16 ib .. 16 ib + 15]."""
    be, bb = BLOCK[t]
    b = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)[:n // be * bb].reshape(-1, bb)
    d = np.ascontiguousarray(b[:, 0:2]).view(np.float16)[:, 0].astype(np.float64)
    if t == NL:
        qs = b[:, 2:18]
        return (d[:, None] * KV[np.concatenate([qs & 15, qs >> 4], axis=1)]).reshape(-1)
    sh = b[:, 2].astype(np.int64) | (b[:, 3].astype(np.int64) << 8)
    out = np.empty((b.shape[0], 8, 32))
    for ib in range(8):
        ls = ((b[:, 4 + ib // 2].astype(np.int64) >> (4 * (ib & 1))) & 15) | (((sh >> (2 * ib)) & 3) << 4)
        q = b[:, 8 + 16 * ib:24 + 16 * ib]
        out[:, ib] = (d * (ls - 32))[:, None] * KV[np.concatenate([q & 15, q >> 4], axis=1)]
    return out.reshape(-1)


@functools.lru_cache(maxsize=None)
def blocks(t, fill, n_rows, K):
    """raw bytes [n_rows][row bytes] and their decoded values [n_rows][K]; every d = a FIELD_VALUES magnitude, its sign alternating from block to block"""
    rng = np.random.default_rng([t, n_rows, K])
    nb, bb = K // BLOCK[t][0], BLOCK[t][1]
    b = rng.integers(0, 256, (n_rows, nb, bb), dtype=np.uint8) if fill == "random" else np.full((n_rows, nb, bb), fill, np.uint8)
    d = np.abs(QB.FIELD_VALUES[rng.integers(0, len(QB.FIELD_VALUES), (n_rows, nb))]) * np.where(np.arange(nb) & 1, -1, 1).astype(np.float16)
    b[:, :, 0:2] = np.ascontiguousarray(d.astype(np.float16))[..., None].view(np.uint8)
    raw = b.reshape(n_rows, nb * bb)
    return raw, decode_iq4(t, raw, n_rows * K).reshape(n_rows, K)


def ratio(t, w, K, got, x, residual=None, what=""):
    x = np.asarray(x, np.float64).reshape(-1, K)
    r = QB.ratio_of(np.asarray(got).reshape(x.shape[0], -1), x @ w.T, np.abs(x) @ np.abs(w).T, K // BLOCK[t][0], residual)
    print("iq4/%s K%d %s: ratio %.4f" % (NAMES[t], K, what, r))
    return r


# (hook, type, N, K, rows per matrix, matrices, forced K split, option: mmq2 = a residual of small integers, matvec = the row preparation in the prologue)
CASES = ([("mul_mat", t, N, K, R, 1, 0, 0) for t in (NL, XS) for N, K, R in ((3, 512, 96), (33, 1024, 70))] + [("mul_mat", NL, 5, 352, 100, 1, 0, 0)]   # N 33: the MFMA route; K 352: 11 blocks
         + [("mmq2", t) + c for t in (NL, XS) for c in QB.MMQ2_SHAPES]
         + [("matvec", t, 1, K, 130, m, 0, fuse) for t in (NL, XS) for K in (512, 5120) for m in (1, 3) for fuse in (0, 1)]
         + [("matvec_rows", t, N, K, 130, 3, 0, 0) for t in (NL, XS) for K in (512, 5120) for N in (1, 3, 4)])


@pytest.mark.parametrize("hook,t,N,K,R,n_mat,ks,opt", CASES, ids=["%s-%s-N%d-K%d-R%d-m%d-ks%d-o%d" % ((c[0], NAMES[c[1]]) + tuple(c[2:])) for c in CASES])
def test_kernel_on_arbitrary_blocks(gpu_lib, hook, t, N, K, R, n_mat, ks, opt):
    """k_mul_mat / the prefill dispatch, k_mmq2_iq4 (generation 2), k_matvec_v2 (prep 2, activation rows 0..5), k_matvec_tn (TN 2, 3, 4): ratio <= 1 for every fill"""
    res = np.random.default_rng(N + K).integers(-3, 4, (n_mat, N, R)).astype(np.float32) if hook == "mmq2" and opt else None
    ratios = {}
    for fill in FILLS:
        raw, w = blocks(t, fill, n_mat * R, K)
        for first in range(6) if hook == "matvec" else (0,):
            x = QB.act_rows(ACT[t], K, N, first)
            if hook == "mul_mat":
                got = gpu_lib.amd_test_mul_mat(t, raw.reshape(-1), K, R, x)[None]
            elif hook == "mmq2":
                got = gpu_lib.amd_test_mmq2(t, raw.reshape(-1), n_mat, K, R, x, residual=res, ks=ks, generation=2)
            elif hook == "matvec":
                got = gpu_lib.amd_test_matvec(t, raw.reshape(-1), n_mat, K, R, x[0], prep=2, fuse=bool(opt)).reshape(n_mat, 1, R)
            else:
                got = gpu_lib.amd_test_matvec_rows(t, raw.reshape(-1), n_mat, K, R, x)
            for m in range(n_mat):
                ratios[(fill, first, m)] = ratio(t, w[m * R:(m + 1) * R], K, got[m], x, None if res is None else res[m].astype(np.float64), "%s %s first%d mat%d" % (hook, fill, first, m))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


@both
@pytest.mark.parametrize("K", [256, 1280])
def test_get_rows(gpu_lib, t, K):
    """k_get_rows / dequant_elem: d * (ls - 32) * kv has at most 11 + 6 + 7 bits, so every gathered element equals the decoder exactly; token -1 and the guard row keep their fill"""
    n, tokens = QB.GET_ROWS_TABLE, QB.GET_ROWS_TOKENS
    for fill in FILLS:
        raw, w = blocks(t, fill, n, K)
        out = gpu_lib.amd_test_get_rows(t, raw.reshape(-1), n, K, tokens)
        for i, tok in enumerate(tokens):
            if tok < 0:
                assert (out[i].view(np.uint32) == 0xFFFFFFFF).all(), (fill, "the row of token -1 was written")
            else:
                assert np.array_equal(out[i].astype(np.float64), w[tok]), (fill, i, int(np.argmax(np.abs(out[i] - w[tok]))))
        assert (out[len(tokens)].view(np.uint32) == 0xFFFFFFFF).all(), (fill, "guard row written")


@functools.lru_cache(maxsize=None)
def iq4_files(d, wtype):   # -> (GGUF file of the type, GGJT Q8_0 twin) of a conditioned tiny model with five-bit block scales
    from minigpt4_cpp_amd import modelgen as G
    src, gguf, twin = (os.path.join(d, "llm_%s.%s" % (wtype, e)) for e in ("bin", "gguf", "q8_0.bin"))
    G.write_llm_file(src, G.tiny_llm(wtype=wtype, n_embd=256, n_layer=2, n_head=4, n_vocab=512), seed=1, std=0.05, d_bits=5, **G.TINY_CONDITIONED)
    G.ggjt_to_gguf(src, gguf)
    G.write_q8_0_twin(src, twin)
    return gguf, twin


@pytest.mark.parametrize("wtype", ["iq4_nl", "iq4_xs"])
def test_gguf_file_logits_and_greedy_tokens(gpu_lib, tiny_files, tmpdir_models, wtype):
    """40-row prompt pass (MFMA route) + 8 greedy steps, fast mode, against the oracle on the Q8_0 twin; IQ4_XS rows are Q8_K, the twin's Q8_0.  Worst on an MI355X: 1.8e-3 (NL), 6.4e-3 (XS)."""
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    from test_gpu_parity import LOGIT_TOL, _rel
    gguf, twin = iq4_files(tmpdir_models, wtype)
    ctx = gpu_lib.minigpt4_model_load(tiny_files[0], gguf, verbosity=1, n_ctx=96, n_batch=64)
    try:
        o = R.OracleLLM(G.read_llm_file(twin), n_ctx=96)
        toks = [1] + [int(v) for v in np.random.default_rng(7).integers(3, 512, 39)]
        gpu_lib.amd_eval_tokens(ctx, toks)
        want, got, errs = o.eval_tokens(toks), gpu_lib.amd_logits(ctx), []
        for step in range(8):
            errs.append(_rel(got, want))
            gid, oid = int(got.argmax()), int(want.argmax())
            assert gid == oid, (step, gid, oid, errs)
            gpu_lib.amd_eval_tokens(ctx, [gid])
            want, got = o.eval_tokens([oid]), gpu_lib.amd_logits(ctx)
        errs.append(_rel(got, want))
        print("iq4/%s whole model: worst logit error %.3e of the largest |logit|" % (wtype, max(errs)))
        assert max(errs) <= LOGIT_TOL, errs
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("B", [2, 5])
def test_batched_steps_equal_single_conversation_runs(gpu_lib, tiny_files, tmpdir_models, B):
    """end_chat_batch on the IQ4_XS file (2: k_matvec_tn, 5: the MFMA kernel on a few rows): every conversation gets the pieces of its own single-conversation run"""
    from test_gpu_batch import PROMPTS, start
    gguf, _ = iq4_files(tmpdir_models, "iq4_xs")
    ctx = gpu_lib.minigpt4_model_load(tiny_files[0], gguf, verbosity=0, n_ctx=256, n_batch=32)
    try:
        def run(prompts):
            start(gpu_lib, ctx, prompts)
            steps = [gpu_lib.amd_end_chat_batch(ctx, list(range(len(prompts))), temp=0.0) for _ in range(8)]
            return [[st[s] for st in steps] for s in range(len(prompts))]
        got = run(PROMPTS[:B])
        for s in range(B):
            gpu_lib.minigpt4_reset_chat(ctx)
            assert got[s] == run(PROMPTS[s:s + 1])[0], s
    finally:
        gpu_lib.minigpt4_free(ctx)
