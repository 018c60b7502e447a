"""The computed exp / SiLU / GELU forms of fast mode (csrc/activations.hpp), pinned to what they claim.

1. Scalar: each function evaluated on the device over all 65 536 fp16 bit patterns (minigpt4_amd_test_activation), once gathering from the oracle's table (must reproduce it
   bit for bit) and once with the null table pointer the engine ships (the contract of activation_ref.py: within one fp16 ulp of the table on every finite argument, at most
   63 of 63 488 arguments different, +-0 / +-inf / NaN as the table).  THE ONLY TOLERANCE OF THIS FILE'S EPILOGUE TESTS LIVES HERE.
2. Every kernel epilogue that calls one of them, driven with BOTH arms through exact pre-activations: a selection weight matrix (W[n][k] = 1 where k == n % K, else 0) makes every
   output sum one fp16 value plus zeros -- exact in fp32 in any accumulation order, tile shape or K split -- so the output must EQUAL table[bits(A)] (table arm) resp. the
   array the scalar hook returned (computed arm: the epilogue is the scalar function and nothing else).
3. The ViT / Q-Former attention kernel (k_attn_vit: the one image-path kernel with a softmax) alone, at the engine's call shapes and at ragged key counts, both exp arms.

Every run writes what it measured next to the other observation records (parity_observed_activation_deviation.json, activation_ref.record);
tests/golden/activation_deviation_observed.json is one GPU box's record."""
import ctypes

import numpy as np
import pytest

import activation_ref as AR
from test_gpu_parity import GEMM_ARMS, MATVEC_CASES

pytestmark = pytest.mark.gpu
WHICH = [AR.GELU, AR.SILU, AR.EXP]
_ids = lambda w: AR.NAMES[w]   # noqa: E731


def _table(which):
    import refcpu as R
    return R.table(which)


@pytest.fixture(scope="module")
def scalar(gpu_lib):
    """which -> the computed form's 65 536 results on this device (uint16 bit patterns)."""
    return {w: gpu_lib.amd_test_activation(w, None) for w in WHICH}


# ---------------------------------------------------------------------------------------------------------------- 1. scalar
@pytest.mark.parametrize("which", WHICH, ids=_ids)
def test_scalar_table_arm_reproduces_the_table(gpu_lib, which):
    table = _table(which)
    AR.assert_table_sanity(which, table)
    got = gpu_lib.amd_test_activation(which, table)
    assert np.array_equal(got, table), [(hex(int(i)), hex(int(got[i])), hex(int(table[i]))) for i in np.nonzero(got != table)[0][:8]]   # all 65 536 patterns, NaNs included


@pytest.mark.parametrize("which", WHICH, ids=_ids)
def test_scalar_computed_arm_meets_the_contract(gpu_lib, scalar, which):
    dev = AR.assert_computed_contract(which, scalar[which], _table(which))
    AR.record("device", AR.NAMES[which], dev)


# ---------------------------------------------------------------------------------------------------------------- 2. epilogues
# The f16 MFMA path keeps fp16 subnormal inputs (measured: a selection GEMM without an epilogue returns all 63 488 finite patterns as they went in), so the sweep covers them.
# One pattern does not arrive bit for bit: -0.  Its product -0 * 1 is added to +0 products / a +0 accumulator, and (-0) + (+0) = +0 in round-to-nearest: the pre-activation
# of an A entry -0 is +0, in ggml's mul_mat as well.  The expectation indexes with +0 there; f(-0) itself is covered by the scalar test.
FINITE_BITS = AR.BITS[AR.FINITE]
# with a bias of 2.0: A + 2 is exact in fp32 when A's last bit is at least 2^-22 (fp32 ulp of 2.0 .. 4.0 is 2^-22; towards 65504 + 2 the 24 bits reach further down than fp16's
# 11): fp16 exponent field >= 3 (2^-12 and up), and zero
BIAS = np.float32(2.0)
BIAS_BITS = AR.BITS[AR.FINITE & ((((AR.BITS >> 10) & 31) >= 3) | ((AR.BITS & 0x7FFF) == 0))]


def _selection(N, K):
    W = np.zeros((N, K), np.float32)
    W[np.arange(N), np.arange(N) % K] = 1.0
    return W


def _operands(M, K, N, bits):
    assert M * K >= bits.size and N >= K            # every pattern is in A, every column of A reaches the output
    a = np.resize(bits, M * K).reshape(M, K)        # padded by repetition
    return a, a.view(np.float16).astype(np.float32), _selection(N, K)


def _pre_bits(a, N, bias):
    """fp16 bit pattern of the pre-activation the epilogue rounds: A[m][n % K] (+ bias, exact by construction); -0 arrives as +0 (above)."""
    x = a[:, np.arange(N) % a.shape[1]].view(np.float16).astype(np.float32)
    if bias is not None:
        y = x + bias
        assert np.array_equal(y.astype(np.float64), x.astype(np.float64) + np.float64(bias))        # the sum is exact in fp32
        x = y
    b = x.astype(np.float16).view(np.uint16)
    return np.where(b == 0x8000, np.uint16(0), b)


def _check_gelu_gemm(gpu_lib, scalar, M, K, N, skinny=False, with_bias=False):
    table = _table(AR.GELU)
    a, A, W = _operands(M, K, N, BIAS_BITS if with_bias else FINITE_BITS)
    bias = np.full(N, BIAS, np.float32) if with_bias else np.zeros(N, np.float32)
    idx = _pre_bits(a, N, BIAS if with_bias else None)
    got = gpu_lib.amd_test_gemm_f16(A, W, bias, True, skinny=skinny, gelu_table=table)
    want = table[idx].view(np.float16).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("table arm", M, K, N, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    got = gpu_lib.amd_test_gemm_f16(A, W, bias, True, skinny=skinny, computed=True)
    want = scalar[AR.GELU][idx].view(np.float16).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("computed arm", M, K, N, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


# (M, K, N): 257 rows -> the dispatcher's small-M tiles (k_gemm_f16 / k_gemm_dma); 1028 x 3730 -> more 128x128 tiles than CUs: k_gemm_f16_big, ragged M and N, one k tile;
# 515 x 130 -> ragged M >= 512 with several k tiles
@pytest.mark.parametrize("with_bias", [False, True], ids=["bias0", "bias2"])
@pytest.mark.parametrize("shape", [(257, 256, 352), (1028, 64, 3730), (515, 128, 130)], ids=lambda s: "M%d_K%d_N%d" % s)
def test_gelu_epilogue_of_the_gemm_is_the_scalar_function(gpu_lib, scalar, shape, with_bias):
    _check_gelu_gemm(gpu_lib, scalar, *shape, with_bias=with_bias)


@pytest.mark.parametrize("with_bias", [False, True], ids=["bias0", "bias2"])
def test_gelu_epilogue_of_the_skinny_gemm_is_the_scalar_function(gpu_lib, scalar, with_bias):
    _check_gelu_gemm(gpu_lib, scalar, 32, 2048, 2048, skinny=True, with_bias=with_bias)      # the Q-Former's M = 32; N % 16 == 0, K % 32 == 0


@pytest.mark.parametrize("arm", GEMM_ARMS)
def test_gelu_epilogue_of_every_gemm_arm_is_the_scalar_function(gpu_lib, scalar, arm):
    """Every tile shape of launch_gemm_f16_arm (k_gemm_f16 3..14, k_gemm_dma 20..31, the large tiles 32..39; an arm that refuses a shape falls back to the default launch)."""
    L = gpu_lib.library
    L.minigpt4_amd_test_set_gemm_arm.argtypes = [ctypes.c_int, ctypes.c_int]
    L.minigpt4_amd_test_set_gemm_arm.restype = None
    try:
        L.minigpt4_amd_test_set_gemm_arm(arm, 0)
        _check_gelu_gemm(gpu_lib, scalar, 257, 256, 352)
        _check_gelu_gemm(gpu_lib, scalar, 515, 128, 130, with_bias=True)
    finally:
        L.minigpt4_amd_test_set_gemm_arm(0, 0)


@pytest.mark.parametrize("shape", [(259, 256, 320), (515, 128, 512)], ids=lambda s: "N%d_K%d_F%d" % s)
def test_silu_epilogue_of_the_f16_pair_launch_is_the_scalar_function(gpu_lib, scalar, shape):
    """k_gemm_dma PAIR: out_h = fp16(silu(w1 x) * (w3 x)).  w1 selects column n % (K - 1) of x, w3 selects the last column, which holds 1.0: the output IS the SiLU entry."""
    M, K, F = shape
    table = _table(AR.SILU)
    assert M * (K - 1) >= FINITE_BITS.size and F >= K - 1
    a = np.empty((M, K), np.uint16)
    a[:, :K - 1] = np.resize(FINITE_BITS, M * (K - 1)).reshape(M, K - 1)
    a[:, K - 1] = 0x3C00                                                                          # 1.0
    x = a.view(np.float16).astype(np.float32)
    w = np.zeros((2 * F, K), np.float16)
    w[np.arange(F), np.arange(F) % (K - 1)] = 1.0
    w[F:, K - 1] = 1.0
    b = a[:, np.arange(F) % (K - 1)]
    idx = np.where(b == 0x8000, np.uint16(0), b)
    for name, kw, ref in (("table arm", {"silu_table": table}, table), ("computed arm", {"computed": True}, scalar[AR.SILU])):
        oh, of = gpu_lib.amd_test_f16_silu_pair(x, w, **kw)
        assert np.array_equal(oh, ref[idx]), (name, shape, int((oh != ref[idx]).sum()))
        assert np.array_equal(of.view(np.uint32), ref[idx].view(np.float16).astype(np.float32).view(np.uint32)), (name, shape, "fp32 product")


# ---- decode: silu(x) * x2 of the stand-alone preparation launch (k_silu_mul_quant: the ONE decode launch with a computed SiLU arm -- the mat-vec's fused prologue and its
# w1 | w3 pair epilogue are handed the table by the engine and gather always; the hook refuses them without one) in front of the decode mat-vec, over the parametrisation and with
# the bar of test_gpu_parity.py::test_decode_matvec_variants_match_oracle (2e-5).  Computed arm: the prepared row comes from the scalar hook's array instead of the table
@pytest.mark.parametrize("wtype,K", MATVEC_CASES)
@pytest.mark.parametrize("arm", ["table", "computed"])
def test_decode_matvec_standalone_silu_preparation(gpu_lib, scalar, wtype, K, arm):
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    from test_gpu_parity import _prepared_row
    t = Q.NAME_TO_TYPE[wtype]
    rng = np.random.default_rng(K * 7 + 3 * 3 + sum(map(ord, wtype)))
    rows = 2300 if K <= 5120 else 1100
    w = (0.03 * rng.standard_normal((rows, K))).astype(np.float32)
    raw = Q.quantize(t, w)
    x = (rng.standard_normal(K) * 3.0).astype(np.float32)
    x2 = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32)
    table = _table(AR.SILU)
    kw, ref = ({"silu_table": table}, table) if arm == "table" else ({"computed": True}, scalar[AR.SILU])
    got = gpu_lib.amd_test_matvec(t, raw, 1, K, rows, x, x2, prep=3, fuse=False, **kw).reshape(-1)
    want = R.mul_mat(t, raw, K, rows, _prepared_row(3, x, x2, ref.view(np.float16))[None, :])[0]
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max(), (wtype, K, arm)


def test_decode_matvec_hook_refuses_the_gathering_launches_without_a_table(gpu_lib):
    from minigpt4_cpp_amd import quants as Q
    raw = Q.quantize(Q.NAME_TO_TYPE["q4_0"], np.zeros((64, 512), np.float32))
    x = np.ones(512, np.float32)
    for kw in ({"prep": 3, "fuse": True}, {"prep": 1, "fuse": False, "epi": 1}):
        with pytest.raises(RuntimeError, match="need a table"):
            gpu_lib.amd_test_matvec(Q.NAME_TO_TYPE["q4_0"], raw, 2 if kw.get("epi") else 1, 512, 32 if kw.get("epi") else 64, x, x, computed=True, **kw)


# ---------------------------------------------------------------------------------------------------------------- 3. attention
def _attn_inputs(heads, hd, nq, nk, batch, seed):
    """Asymmetric values (V has a mean, so a probability that lands on the wrong key or a pad key shows) and a few large scores (some query and key rows are scaled up, so
    a wrong maximum overflows or flattens a row)."""
    rng = np.random.default_rng(seed)
    D = heads * hd
    q = rng.standard_normal((batch * nq, D)).astype(np.float32)
    k = rng.standard_normal((batch * nk, D)).astype(np.float32)
    v = (0.5 + rng.standard_normal((batch * nk, D)) * np.linspace(0.5, 2.0, D)).astype(np.float32)
    q[rng.integers(0, batch * nq, max(1, batch * nq // 8))] *= 4.0
    k[rng.integers(0, batch * nk, max(1, batch * nk // 8))] *= 3.0
    k[batch * nk - 1] *= 2.0                                                   # the LAST key matters (ragged tiles)
    return q, k, v


def _attn_refs(q, k, v, heads, hd, nq, nk, batch, q_prescale, score_div):
    """(a) plain float64 softmax attention; (b) the same with ggml's rounding points: fp32 pre-scaled q, the exponential from the oracle's fp16 table on the fp16-rounded s - max,
    p = e * float32(1 / sum) in fp32."""
    etab = _table(AR.EXP).view(np.float16).astype(np.float64)
    D = heads * hd
    qs = (q * np.float32(q_prescale)) if q_prescale != 0.0 else q
    a, b = np.empty((batch * nq, D)), np.empty((batch * nq, D))
    for z in range(batch):
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            Q, K, V = qs[z * nq:(z + 1) * nq, c].astype(np.float64), k[z * nk:(z + 1) * nk, c].astype(np.float64), v[z * nk:(z + 1) * nk, c].astype(np.float64)
            s = Q @ K.T
            if score_div != 0.0:
                s = s / score_div
            d = s - s.max(axis=1, keepdims=True)
            pa = np.exp(d)
            a[z * nq:(z + 1) * nq, c] = (pa / pa.sum(axis=1, keepdims=True)) @ V
            e = etab[d.astype(np.float32).astype(np.float16).view(np.uint16)]
            inv = (1.0 / e.sum(axis=1, keepdims=True)).astype(np.float32)
            p = (e.astype(np.float32) * inv).astype(np.float64)
            b[z * nq:(z + 1) * nq, c] = p @ V
    return a, b


VIT, QF = 1.0 / np.sqrt(88.0), 8.0
# (name, heads, hd, nq, nk, batch, q_prescale, score_div): the engine's four call shapes, then ragged key counts for both head sizes (nk <= 64 with hd 64: the short-key
# instantiation; nk % 16 != 0: the key mask; 320: the kernel's limit)
ATTN_CASES = [("vit", 16, 88, 257, 257, 1, VIT, 0.0), ("vit_b4", 16, 88, 257, 257, 4, VIT, 0.0),
              ("qformer_self", 12, 64, 32, 32, 1, 0.0, QF), ("qformer_self_b4", 12, 64, 32, 32, 4, 0.0, QF),
              ("qformer_cross", 12, 64, 32, 257, 1, 0.0, QF), ("qformer_cross_b4", 12, 64, 32, 257, 4, 0.0, QF)]
ATTN_CASES += [("ragged88_nk%d" % nk, 16, 88, 40, nk, 2, VIT, 0.0) for nk in (1, 15, 17, 255, 320)]
ATTN_CASES += [("ragged64_nk%d" % nk, 12, 64, 32, nk, 2, 0.0, QF) for nk in (1, 15, 17, 255, 320)]


@pytest.mark.parametrize("arm", ["table", "computed"])
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: c[0])
def test_attn_vit_kernel_alone(gpu_lib, case, arm):
    """|got - (b)| <= 2 max|(a) - (b)|: the bar is the noise of the reference's own table arithmetic on these inputs, doubled -- the kernel's fp32 scores can flip the fp16
    rounding of an exponential's argument that (b) rounds the other way.  A dropped key tile, a wrong head stride or an unmasked pad key is orders of magnitude above it.
    Query tiles per workgroup and the two input layouts must not change a bit."""
    name, heads, hd, nq, nk, batch, q_prescale, score_div = case
    q, k, v = _attn_inputs(heads, hd, nq, nk, batch, seed=sum(map(ord, name)))
    a, b = _attn_refs(q, k, v, heads, hd, nq, nk, batch, q_prescale, score_div)
    bar = 2.0 * np.abs(a - b).max()
    etab = _table(AR.EXP) if arm == "table" else None
    got, got_h = gpu_lib.amd_test_attn_f32(q, k, v, heads, hd, nq, nk, batch, q_prescale, score_div, head_major=False, qt=0, exp_table=etab)
    err = float(np.abs(got.astype(np.float64) - b).max())
    print(f"{name} [{arm}]: max|got - b| = {err:.3e}, bar = {bar:.3e}, max|b| = {np.abs(b).max():.3e}")
    AR.record("attn_vit_" + arm, name, {"err": err, "bar": float(bar)})
    assert np.isfinite(got).all()
    assert err <= bar, (name, arm, err, bar)
    assert np.array_equal(got_h, got.astype(np.float16).view(np.uint16))                          # the fp16 copy the engine consumes
    for head_major in (False, True):
        for qt in (0, 1, 2, 4):
            if not head_major and qt == 0:
                continue
            g2, h2 = gpu_lib.amd_test_attn_f32(q, k, v, heads, hd, nq, nk, batch, q_prescale, score_div, head_major=head_major, qt=qt, exp_table=etab)
            assert np.array_equal(g2.view(np.uint32), got.view(np.uint32)) and np.array_equal(h2, got_h), (name, arm, "head_major" if head_major else "row_major", qt)
