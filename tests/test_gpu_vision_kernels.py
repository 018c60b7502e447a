"""The kernels that sit BETWEEN the image encoder's GEMMs, one launch each, against independent references (csrc/vision_kernels.hip through the hooks of
include/minigpt4_amd_test.h): k_layernorm<3|6|8>, k_splitk_reduce_ln<2|4|8|12, 3|6|8>, the split-K forms of k_gemm_f16 / k_gemm_dma / k_gemm_f16_skinny, the head-major output
map of launch_gemm_f16_head_major, k_im2col, k_assemble and k_lin_epilogue.

Most of what these kernels do is address arithmetic or a fixed sequence of IEEE fp32 operations (the library is built with -ffp-contract=off), so most assertions here are
bit for bit.  The one tolerance is the LayerNorm bound of tests/vision_kernel_refs.py (ln_bound: derived there, checked without a GPU by test_cpu_vision_kernel_refs.py);
the random-operand GEMM check uses the suite's existing fp16-GEMM rule (test_gpu_parity._rel < 2e-5).

Every LayerNorm / reduce case writes its largest observed |error| / bound next to the suite's other observation records (parity_observed_vision_kernels.json);
tests/golden/vision_kernels_observed.json is one GPU box's record (worst: 0.434 for k_layernorm, 0.485 for k_splitk_reduce_ln).  The assertions stay the derived bound."""
import numpy as np
import pytest

import vision_kernel_refs as V
from test_gpu_parity import _rel

pytestmark = pytest.mark.gpu

FILL32, FILL16 = np.uint32(0xFFFFFFFF), np.uint16(0xFFFF)            # the hooks' 0xFF prefill as seen through an fp32 / fp16 output
_OBSERVED = {}


def _record(section, name, ratio):
    from test_gpu_headline import _dump
    _OBSERVED.setdefault(section, {})[name] = float(ratio)
    _dump("vision_kernels", _OBSERVED)


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _untouched(a):
    """an output array of the wrappers that the hook did not copy back"""
    from minigpt4_cpp_amd import minigpt4_library as ML
    return bool((a.view(np.uint8) == ML.MiniGPT4SharedLibrary.HOOK_FILL).all())


def _guard_ok(a):
    """the hook's guard row (the last one) still holds the 0xFF prefill"""
    return bool((a[-1].view(np.uint8) == 0xFF).all())


def _f16_bits(a):
    return a.astype(np.float16).view(np.uint16)                       # numpy rounds fp32 -> fp16 to nearest even, as v_cvt_f16_f32 does


def _ln_ratio(got, x, w, b):
    """max |got - ln_f64(x)| / bound over all elements (0 / 0 = 0)"""
    want, _, _ = V.ln_f64(x, w, b)
    bound = V.ln_bound(x, w, b)
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


# =========================================================================================================================== LayerNorm
LN_N = [1, 176, 255, 256, 257, 768, 769, 1408, 1536, 1537, 2047, 2048]          # 768 | 769 and 1536 | 1537: the edges of the size classes <3>, <6>, <8>; 2048: the limit
# rows of V.FAMILIES per launch: 3-row launches (more than one workgroup, every family in one of them) and each family alone
LN_GROUPS = [(0, 1, 4), (2, 3, 0), (0,), (1,), (2,), (3,), (4,)]
ZERO = V.FAMILIES.index("zero")


@pytest.mark.parametrize("n", LN_N)
def test_layernorm_kernel_alone(gpu_lib, n):
    x_all, w, b_all = V.ln_case(n)
    worst = 0.0
    for group in LN_GROUPS:
        x = np.ascontiguousarray(x_all[list(group)])
        rows = len(group)
        for b in (b_all, None):
            tag = (n, group, b is not None)
            rc, out, out_h = gpu_lib.amd_test_layernorm(x, w, b)
            assert rc == 0, (tag, rc, gpu_lib._err())
            assert _guard_ok(out) and _guard_ok(out_h), tag
            assert np.isfinite(out[:rows]).all(), tag
            ratio = _ln_ratio(out[:rows], x, w, b)
            print(f"layernorm n={n} rows={group} b={b is not None}: max |error| / bound = {ratio:.3f}")
            worst = max(worst, ratio)
            assert ratio <= 1.0, (tag, ratio)
            if ZERO in group:                                                      # variance 0, eps decides: exactly b (w * 0 without one)
                assert np.array_equal(out[group.index(ZERO)], b if b is not None else np.zeros(n, np.float32)), tag
            assert np.array_equal(out_h[:rows], _f16_bits(out[:rows])), tag         # the fp16 copy is the rounding of the fp32 result of the same launch
            rc, o2, none = gpu_lib.amd_test_layernorm(x, w, b, want_out_h=False)
            assert rc == 0 and none is None and _same_bits(o2, out), tag
            rc, none, h2 = gpu_lib.amd_test_layernorm(x, w, b, want_out=False)
            assert rc == 0 and none is None and np.array_equal(h2, out_h), tag
            # sequential_sums: ggml_norm's two loops literally -> the emulation with one float64 accumulator in element order, bit for bit
            rc, so, sh = gpu_lib.amd_test_layernorm(x, w, b, sequential=True)
            assert rc == 0 and _guard_ok(so) and _guard_ok(sh), tag
            want = V.ln_f32_emulated(x, w, b, sequential=True)
            assert _same_bits(so[:rows], want), (tag, int((_bits(so[:rows]) != _bits(want)).sum()))
            assert np.array_equal(sh[:rows], _f16_bits(so[:rows])), tag
    _record("layernorm", f"n{n}", worst)


def test_layernorm_refuses_a_row_longer_than_2048(gpu_lib):
    x, w, b = V.ln_case(2049)
    for kw in ({}, {"sequential": True}):
        rc, out, out_h = gpu_lib.amd_test_layernorm(x[:3], w, b, **kw)
        assert rc == 3, rc
        assert _untouched(out) and _untouched(out_h)
    x, w, b = V.ln_case(2048)                                                    # the refusal left nothing behind: the next call works
    rc, out, out_h = gpu_lib.amd_test_layernorm(x[:3], w, b)
    assert rc == 0 and _ln_ratio(out[:3], x[:3], w, b) <= 1.0


# =========================================================================================================================== slab reduce + LayerNorm
RLN_SLABS = [1, 2, 3, 4, 5, 8, 9, 12]                                          # 2 | 3, 4 | 5, 8 | 9: the edges of the slab-count classes <2>, <4>, <8>, <12>; 12: the limit
RLN_N = [176, 768, 769, 1408, 1537, 2048]
# (bias, residual, in_place, LayerNorm, ln_b, x_out wanted): the ViT blocks' call first; the Q-Former's (no x_out); ln_w NULL (x_out only)
RLN_COMBOS = [(1, 1, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 0, 1, 1, 0), (1, 0, 0, 1, 1, 1), (0, 1, 0, 1, 1, 1), (0, 0, 0, 1, 0, 1), (1, 1, 1, 0, 0, 1), (0, 0, 0, 0, 0, 1)]


def _padded(slabs, stride):
    """[n_slabs][rows][n] -> [n_slabs][stride] with NaN in the padding between the slabs"""
    p = np.full((slabs.shape[0], stride), np.nan, np.float32)
    p[:, :slabs[0].size] = slabs.reshape(slabs.shape[0], -1)
    return p


@pytest.mark.parametrize("n", RLN_N)
@pytest.mark.parametrize("n_slabs", RLN_SLABS)
def test_splitk_reduce_ln_kernel_alone(gpu_lib, n_slabs, n):
    rng = np.random.default_rng(7000 + 13 * n_slabs + n)
    w, b = V.ln_params(rng, n)
    worst = 0.0
    for rows in (1, 3):
        slabs, bias, residual = V.reduce_case(rng, n_slabs, rows, n)
        for stride in (rows * n, rows * n + 64):
            for (has_bias, has_res, in_place, ln, has_lb, want_x) in RLN_COMBOS:
                tag = (n_slabs, n, rows, stride, has_bias, has_res, in_place, ln, has_lb, want_x)
                bias_, res_ = (bias if has_bias else None), (residual if has_res else None)
                lw, lb = (w if ln else None), (b if ln and has_lb else None)
                rc, x_out, ln_out, ln_out_h = gpu_lib.amd_test_splitk_reduce_ln(_padded(slabs, stride), rows, n, bias_, res_, bool(in_place), lw, lb, want_x=bool(want_x))
                assert rc == 0, (tag, rc, gpu_lib._err())
                want_xv = V.reduce_f32_emulated(slabs, bias_, res_)
                if want_x:
                    assert _guard_ok(x_out), tag
                    assert _same_bits(x_out[:rows], want_xv), (tag, int((_bits(x_out[:rows]) != _bits(want_xv)).sum()))       # no NaN of the padding, every addition in order
                if not ln:
                    assert ln_out is None and ln_out_h is None
                    continue
                assert _guard_ok(ln_out) and _guard_ok(ln_out_h), tag
                assert np.isfinite(ln_out[:rows]).all(), tag
                ratio = _ln_ratio(ln_out[:rows], want_xv, lw, lb)                    # against float64 on that exact x_out
                worst = max(worst, ratio)
                assert ratio <= 1.0, (tag, ratio)
                assert np.array_equal(ln_out_h[:rows], _f16_bits(ln_out[:rows])), tag
    # variance 0 behind the reduce: an all-zero row (every slab zero) and a constant row (slab 0 constant, the others zero) give exactly b; a third row with a spread
    deg = np.zeros((n_slabs, 3, n), np.float32)
    deg[0, 1] = np.float32(rng.uniform(-3.0, 3.0))
    deg[:, 2] = rng.standard_normal((n_slabs, n))
    rc, x_out, ln_out, ln_out_h = gpu_lib.amd_test_splitk_reduce_ln(deg.reshape(n_slabs, -1), 3, n, ln_w=w, ln_b=b)
    assert rc == 0 and _same_bits(x_out[:3], V.reduce_f32_emulated(deg)), (n_slabs, n)
    assert np.array_equal(ln_out[0], b) and np.array_equal(ln_out[1], b), (n_slabs, n)
    ratio = _ln_ratio(ln_out[:3], x_out[:3], w, b)
    worst = max(worst, ratio)
    assert ratio <= 1.0, (n_slabs, n, ratio)
    if n_slabs == 1:                                                                # one slab, no bias, no residual: the LayerNorm kernel's bits on the same rows
        fam_all = V.row_families(rng, n)
        for group in LN_GROUPS:
            fam, rows = np.ascontiguousarray(fam_all[list(group)]), len(group)
            rc, x_out, ln_out, ln_out_h = gpu_lib.amd_test_splitk_reduce_ln(fam.reshape(1, -1), rows, n, ln_w=w, ln_b=b)
            rc2, out, out_h = gpu_lib.amd_test_layernorm(fam, w, b)
            assert rc == 0 and rc2 == 0
            assert _same_bits(x_out[:rows], fam) and _same_bits(ln_out, out) and np.array_equal(ln_out_h, out_h), (n, group)
    print(f"splitk_reduce_ln n_slabs={n_slabs} n={n}: max |error| / bound = {worst:.3f}")
    _record("splitk_reduce_ln", f"z{n_slabs}_n{n}", worst)


def test_splitk_reduce_ln_refuses_13_slabs_and_long_rows(gpu_lib):
    rng = np.random.default_rng(5)
    for n_slabs, n in ((13, 176), (2, 2049), (12, 2049)):
        slabs, bias, residual = V.reduce_case(rng, n_slabs, 3, n)
        w, b = V.ln_params(rng, n)
        rc, x_out, ln_out, ln_out_h = gpu_lib.amd_test_splitk_reduce_ln(slabs.reshape(n_slabs, -1), 3, n, bias, residual, False, w, b)
        assert rc == 3, (n_slabs, n, rc)
        assert _untouched(x_out) and _untouched(ln_out) and _untouched(ln_out_h)


# =========================================================================================================================== split-K GEMM
def _exact_operands(rng, M, N, K):
    """A: integers in [-3, 3]; W from {-1, -1/2, 0, 1/2, 1}: every partial sum is a multiple of 1/2 below 2^15 -- exact in fp32 in ANY order, so a slab has ONE right value."""
    A = rng.integers(-3, 4, (M, K)).astype(np.float32)
    W = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32), (N, K))
    assert 3 * K < 2 ** 15
    return A, W


def _slab_products(A, W, kps, slices):
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    K = A.shape[1]
    return np.stack([A64[:, z * kps:min(K, (z + 1) * kps)] @ W64[:, z * kps:min(K, (z + 1) * kps)].T for z in range(slices)])


def _ceil(a, b):
    return -(-a // b)


# (M, N, K, slices wanted, slices used, form).  64x64: (257, 176, 1408, 4) -- the last slice is 2 of 11 k tiles; (33, 64, 256, 3) -- only 2 slices can multiply something.
# From 384 rows on launch_gemm_f16_splitk takes the ring tiles (128x128; 256x128 from 640 rows) when both forms cut K at the same columns: K % 64 == 0 and
# ceil(ceil(K / 128) / s) * 128 == ceil((K / 64) / s) * 64
SPLITK_CASES = [(257, 176, 1408, 2, 2, "64x64"), (257, 176, 1408, 4, 4, "64x64"), (70, 96, 384, 2, 2, "64x64"), (33, 64, 256, 3, 2, "64x64"),
                (514, 192, 512, 2, 2, "ring128x128"), (771, 192, 512, 2, 2, "ring256x128"), (771, 320, 1024, 4, 4, "ring256x128")]


@pytest.mark.parametrize("case", SPLITK_CASES, ids=lambda c: "M%d_N%d_K%d_s%d" % c[:4])
def test_splitk_gemm_slabs_are_the_slice_products(gpu_lib, case):
    M, N, K, wanted, used, form = case
    kps = _ceil(_ceil(K, 128), used) * 128
    ring = K % 64 == 0 and kps == _ceil(K // 64, used) * 64                        # the launcher's rule, restated: the shapes named "ring" must reach that form
    assert form == ("64x64" if M < 384 or not ring else "ring128x128" if M < 640 else "ring256x128"), case
    A, W = _exact_operands(np.random.default_rng(M + N + K + wanted), M, N, K)
    want = _slab_products(A, W, kps, used)
    L = gpu_lib.library
    got = {}
    try:
        for xcd in (1, 0):                                                          # both workgroup -> (tile, slice) mappings
            L.minigpt4_amd_test_set_splitk_xcd(xcd)
            rc, slabs, n_used = gpu_lib.amd_test_gemm_f16_splitk(A, W, wanted)
            assert rc == 0, (case, xcd, rc, gpu_lib._err())
            assert n_used == used, (case, n_used)
            assert _untouched(slabs[used:]), case
            bad = slabs[:used].astype(np.float64) != want
            assert not bad.any(), (case, xcd, int(bad.sum()), [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]])
            got[xcd] = slabs
    finally:
        L.minigpt4_amd_test_set_splitk_xcd(1)
    assert _same_bits(got[0], got[1]), case


SKINNY_CASES = [(16, 64, 2), (48, 160, 3), (768, 768, 2), (768, 3072, 4), (32, 384, 12)]      # (N, K, slices); (48, 160, 3): slices of 64, 64 and 32 columns


@pytest.mark.parametrize("case", SKINNY_CASES, ids=lambda c: "N%d_K%d_s%d" % c)
def test_skinny_splitk_gemm_slabs_are_the_slice_products(gpu_lib, case):
    N, K, slices = case
    kps = _ceil(K // 32, slices) * 32
    for M in (1, 32, 33, 64, 65):                                                   # 32 | 33: the 32-row and the 64-row workgroup; 65: a second row tile
        A, W = _exact_operands(np.random.default_rng(M * 131 + N + K + slices), M, N, K)
        rc, slabs, used = gpu_lib.amd_test_gemm_f16_splitk(A, W, slices, skinny=True)
        assert rc == 0 and used == slices, (case, M, rc, used, gpu_lib._err())
        bad = slabs.astype(np.float64) != _slab_products(A, W, kps, slices)
        assert not bad.any(), (case, M, int(bad.sum()), [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]])


@pytest.mark.parametrize("case", [(8, 24, 64, 2), (8, 16, 48, 2), (8, 16, 64, 1), (8, 16, 64, 13), (8, 48, 160, 4)], ids=lambda c: "M%d_N%d_K%d_s%d" % c)
def test_skinny_splitk_gemm_refusals(gpu_lib, case):
    """N % 16, K % 32, fewer than 2 or more than 12 slices, and (K = 160, 4 slices): 5 k-steps in slices of 2 leave the fourth slice empty."""
    M, N, K, slices = case
    A, W = _exact_operands(np.random.default_rng(1), M, N, K)
    rc, slabs, used = gpu_lib.amd_test_gemm_f16_splitk(A, W, slices, skinny=True)
    assert rc == 4, (case, rc)
    assert _untouched(slabs) and used == -1


# (M, N, K, slices, skinny): one shape per form -- 64x64 tiles with a short last slice, the 256x128 ring tiles, the skinny kernel with a second row tile
@pytest.mark.parametrize("case", [(257, 176, 1408, 4, False), (771, 320, 1024, 4, False), (65, 768, 3072, 4, True)], ids=lambda c: "M%d_N%d_K%d_s%d_%s" % c)
def test_splitk_gemm_random_operands_and_the_reduce_that_follows(gpu_lib, case):
    M, N, K, slices, skinny = case
    rng = np.random.default_rng(M * 7 + K)                                          # the operands of test_gpu_parity.test_gemm_f16_mfma
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (0.1 * rng.standard_normal((N, K))).astype(np.float32)
    rc, slabs, used = gpu_lib.amd_test_gemm_f16_splitk(A, W, slices, skinny=skinny)
    assert rc == 0 and used == slices, (case, rc, used)
    ref = A.astype(np.float16).astype(np.float64) @ W.astype(np.float16).astype(np.float64).T
    total = slabs.astype(np.float64).sum(0)
    print(f"split-K GEMM {case}: rel = {_rel(total, ref):.3e}")
    assert _rel(total, ref) < 2e-5, (case, _rel(total, ref))
    bias = rng.standard_normal(N).astype(np.float32)
    residual = (3.0 * rng.standard_normal((M, N))).astype(np.float32)
    rc, x_out, _, _ = gpu_lib.amd_test_splitk_reduce_ln(slabs.reshape(slices, -1), M, N, bias, residual, True)
    assert rc == 0 and _guard_ok(x_out), (case, rc)
    assert _same_bits(x_out[:M], V.reduce_f32_emulated(slabs, bias, residual)), case


# =========================================================================================================================== head-major output map
def _head_major(C, D, hd):
    """out[which][head][r][d] = C[r][which * D + head * hd + d]"""
    M = C.shape[0]
    return np.ascontiguousarray(C.reshape(M, 3, D // hd, hd).transpose(1, 2, 0, 3))


@pytest.mark.parametrize("case", [(257, 176, 88, 176), (70, 128, 64, 64), (514, 352, 88, 352)], ids=lambda c: "M%d_D%d_hd%d_K%d" % c)
def test_head_major_gemm_is_the_row_major_gemm_permuted(gpu_lib, case):
    M, D, hd, K = case
    rng = np.random.default_rng(sum(case))
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (0.1 * rng.standard_normal((3 * D, K))).astype(np.float32)
    bias = rng.standard_normal(3 * D).astype(np.float32)
    for b in (bias, None):
        rc, out = gpu_lib.amd_test_gemm_f16_head_major(A, W, b, D, hd)
        assert rc == 0, (case, rc, gpu_lib._err())
        C = gpu_lib.amd_test_gemm_f16(A, W, np.zeros(3 * D, np.float32) if b is None else b)
        guard_lo, body, guard_hi = out[:3 * D], out[3 * D:-3 * D], out[-3 * D:]
        assert (_bits(guard_lo) == FILL32).all() and (_bits(guard_hi) == FILL32).all(), case       # nothing written outside [3][D / hd][M][hd]
        assert _same_bits(body.reshape(3, D // hd, M, hd), _head_major(C, D, hd)), (case, b is not None)
    Ae, We = _exact_operands(rng, M, 3 * D, K)
    be = (rng.integers(-4, 5, 3 * D) * 0.5).astype(np.float32)
    rc, out = gpu_lib.amd_test_gemm_f16_head_major(Ae, We, be, D, hd)
    assert rc == 0
    want = _head_major(Ae.astype(np.float64) @ We.astype(np.float64).T + be, D, hd)
    assert np.array_equal(out[3 * D:-3 * D].reshape(want.shape).astype(np.float64), want), case


def test_head_major_gemm_refuses_a_head_size_that_does_not_divide(gpu_lib):
    A, W = _exact_operands(np.random.default_rng(2), 70, 3 * 128, 64)
    rc, out = gpu_lib.amd_test_gemm_f16_head_major(A, W, None, 128, 48)
    assert rc == 3 and _untouched(out)


# =========================================================================================================================== im2col / assemble / lin_epilogue
def _distinct_fp16_image(B, seed):
    """[B][3][224][224] fp32 of fp16-exact values.  An image has more pixels than fp16 has values, so: the 50176 pixels of a PLANE get distinct finite values, and any two
    planes of the batch hold them in a different rotation (the same position never has the same value in two planes) -- a wrong pixel, channel or image shows."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    vals = bits[((bits >> 10) & 31) != 31]
    vals = vals[vals != 0x8000]                                                    # -0 == +0 as a value
    rng = np.random.default_rng(seed)
    vals = rng.permutation(vals)[:224 * 224].view(np.float16).astype(np.float32)
    assert np.unique(vals).size == 224 * 224
    planes = [np.roll(vals, p * 5003) for p in range(B * 3)]                         # 5003 is coprime to 50176: no two of the (at most 48) rotations agree anywhere
    return np.stack(planes).reshape(B, 3, 224, 224)


@pytest.mark.parametrize("B", [1, 3])
def test_im2col_is_a_gather(gpu_lib, B):
    img = _distinct_fp16_image(B, 17 + B)
    rc, got = gpu_lib.amd_test_im2col(img, 592)
    assert rc == 0, (rc, gpu_lib._err())
    # patches[b * 256 + oh * 16 + ow][c * 196 + kh * 14 + kw] = img[b][c][oh * 14 + kh][ow * 14 + kw]
    want = img.reshape(B, 3, 16, 14, 16, 14).transpose(0, 2, 4, 1, 3, 5).reshape(B * 256, 588).astype(np.float16).view(np.uint16)
    assert np.array_equal(got[:-1, :588], want), int((got[:-1, :588] != want).sum())
    assert (got[:-1, 588:] == 0).all()                                              # the zero padding of the patch embedding's K
    assert (got[-1] == FILL16).all()


@pytest.mark.parametrize("B", [1, 2])
def test_assemble_embeddings(gpu_lib, B):
    D = 176
    rng = np.random.default_rng(23 + B)
    cls_token = rng.standard_normal(D).astype(np.float32)
    cls_token[5] = -0.0
    pe = (rng.standard_normal((B * 256, D)) * np.linspace(0.1, 30.0, D)).astype(np.float32)
    pos = rng.standard_normal((257, D)).astype(np.float32)
    pos[0, 5] = -0.0                                                                # (0.0f + -0) + -0 = +0: the kernel's literal 0.0f + base
    rc, got = gpu_lib.amd_test_assemble(cls_token, pe, pos)
    assert rc == 0, (rc, gpu_lib._err())
    want = np.empty((B, 257, D), np.float32)
    want[:, 0] = (np.float32(0.0) + cls_token) + pos[0]                              # row 0 of every image comes from cls
    want[:, 1:] = (np.float32(0.0) + pe.reshape(B, 256, D)) + pos[1:]
    assert _same_bits(got[:-1], want.reshape(B * 257, D)), int((_bits(got[:-1]) != _bits(want.reshape(B * 257, D))).sum())
    assert (_bits(got[-1]) == FILL32).all()


@pytest.mark.parametrize("has_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("gelu", [False, True], ids=["nogelu", "gelu"])
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
def test_lin_epilogue(gpu_lib, has_bias, gelu, has_res):
    import refcpu as R
    rows, n = 5, 177                                                                # 885 elements: three full workgroups and a ragged fourth; bias index = i % n
    rng = np.random.default_rng(31)
    y = (2.0 * rng.standard_normal((rows, n))).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32) if has_bias else None
    residual = (40.0 + rng.standard_normal((rows, n))).astype(np.float32) if has_res else None
    table = R.table(0) if gelu else None
    v = y
    if has_bias:
        v = bias + v
    if gelu:
        v = table[_f16_bits(v)].view(np.float16).astype(np.float32)                 # gathered through the fp16 bits of bias + y
    if has_res:
        v = residual + v
    assert v.dtype == np.float32
    rc, out, out_h = gpu_lib.amd_test_lin_epilogue(y, bias, residual, table)
    assert rc == 0, (rc, gpu_lib._err())
    assert _same_bits(out[:rows], v) and np.array_equal(out_h[:rows], _f16_bits(v))
    assert _guard_ok(out) and _guard_ok(out_h)
    rc, o2, none = gpu_lib.amd_test_lin_epilogue(y, bias, residual, table, want_out_h=False)
    assert rc == 0 and none is None and _same_bits(o2, out)
    rc, none, h2 = gpu_lib.amd_test_lin_epilogue(y, bias, residual, table, want_out=False)
    assert rc == 0 and none is None and np.array_equal(h2, out_h)
