"""The references of tests/test_gpu_vision_kernels.py checked against each other, without a GPU (tests/vision_kernel_refs.py).

On the very rows the GPU tests feed k_layernorm / k_splitk_reduce_ln -- every row length, every input family -- the statement-by-statement fp32 emulation of the kernel
must stay inside the derived bound against the float64 LayerNorm (so the bound does not ask more of the kernel than fp32 arithmetic in the kernel's order can give), must
NOT stay inside a fiftieth of it (so the bound is not vacuous), and three deliberately wrong LayerNorms must be caught by it."""
import numpy as np
import pytest

import vision_kernel_refs as V

LN_N = [1, 176, 255, 256, 257, 768, 769, 1408, 1536, 1537, 2047, 2048]          # = test_gpu_vision_kernels.LN_N
DEGENERATE = ("constant", "zero")                                               # x - mean is exactly 0 in fp32 and in float64: the result is b, the error 0


def _ratio(got, x, w, b):
    """per row: max_i |got - ln_f64| / bound (0 / 0 = 0, e / 0 = inf)"""
    want, _, _ = V.ln_f64(x, w, b)
    bound = V.ln_bound(x, w, b)
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return r.max(-1)


def _case(n, with_b=True):
    x, w, b = V.ln_case(n)
    return x, w, (b if with_b else None)


@pytest.mark.parametrize("sequential", [False, True], ids=["tree", "sequential"])
@pytest.mark.parametrize("with_b", [True, False], ids=["b", "nob"])
@pytest.mark.parametrize("n", LN_N)
def test_emulated_layernorm_is_inside_the_bound_on_every_family(n, with_b, sequential):
    x, w, b = _case(n, with_b)
    r = _ratio(V.ln_f32_emulated(x, w, b, sequential=sequential), x, w, b)
    assert (r <= 1.0).all(), dict(zip(V.FAMILIES, r))
    got = V.ln_f32_emulated(x, w, b, sequential=sequential)
    zero = V.FAMILIES.index("zero")
    assert np.array_equal(got[zero], b if with_b else np.zeros(n, np.float32))          # the all-zero row gives exactly b
    assert np.array_equal(got[V.FAMILIES.index("constant")], got[zero])               # ... and so does a constant row: eps decides, the mean is exact


@pytest.mark.parametrize("n", [k for k in LN_N if k > 1])
def test_bound_is_not_vacuous(n):
    """On every family whose rows have a spread the emulation uses more than a fiftieth of the bound (a row of one element, a constant row and a zero row are exact)."""
    x, w, b = _case(n)
    r = _ratio(V.ln_f32_emulated(x, w, b), x, w, b)
    for name, v in zip(V.FAMILIES, r):
        if name not in DEGENERATE:
            assert v > 1.0 / 50.0, (n, name, v)
    assert r.max() > 1.0 / 50.0


@pytest.mark.parametrize("name", sorted(V.PERTURBED))
def test_perturbed_layernorm_is_caught(name):
    """Each wrong LayerNorm leaves the bound somewhere on the GPU tests' inputs.  Where: a variance taken without the mean, on every row with a mean; eps 1e-6, on the
    unit-spread rows at every n > 1 (s moves by 4.5e-6 relative against 20 u = 1.2e-6); a mean summed in fp32, on the CONSTANT rows whose fp32 sum is inexact -- x - mean
    is then a rounding error instead of 0 and 1 / sqrt(eps) = 316 magnifies it (on the mean-40 rows a pairwise fp32 mean is off by about u |mu|, which the bound's
    2 u |mu| / s term admits: there the kernel's float64 sums are not needed for THIS bound, and the assertion does not pretend otherwise)."""
    caught = {}
    for n in LN_N:
        x, w, b = _case(n)
        r = _ratio(V.PERTURBED[name](x, w, b), x, w, b)
        for fam, v in zip(V.FAMILIES, r):
            if v > 1.0:
                caught.setdefault(fam, []).append(n)
    print(name, caught)
    assert caught, name
    if name == "eps_1e-6":
        assert caught["normal"] == [k for k in LN_N if k > 1] and caught["residual_stream"] == caught["normal"]
    if name == "variance_without_mean":
        assert caught["residual_stream"] == [k for k in LN_N if k > 1]
    if name == "mean_in_fp32":
        assert len(caught.get("constant", [])) >= 2


def test_sequential_sum_is_one_accumulator_in_element_order():
    """np.cumsum adds left to right with one accumulator; the emulation's `sequential` form must equal a literal loop (a pairwise np.sum does not, on a row built to show it)."""
    x = np.array([[2.0 ** 53, 1.0, 1.0, -2.0 ** 53] + [0.0] * 12], np.float64)
    assert V._sum64(x, True)[0, 0] == 0.0                                             # ((2^53 + 1) + 1) - 2^53 = 0 with one accumulator: each + 1 is lost
    rng = np.random.default_rng(3)
    x = (40.0 + rng.standard_normal((2, 1408))).astype(np.float32)
    for r in range(2):
        a = np.float64(0.0)
        for v in x[r]:
            a += np.float64(v)
        assert V._sum64(x, True)[r, 0] == a


def test_reduce_emulation_order_matters_and_is_fp32():
    """The slabs the GPU tests draw (a different magnitude per slab) make the order of additions visible: reversed slab order, or bias added last, changes bits."""
    rng = np.random.default_rng(11)
    slabs, bias, res = V.reduce_case(rng, 5, 3, 769)
    want = V.reduce_f32_emulated(slabs, bias, res)
    assert want.dtype == np.float32
    assert not np.array_equal(want, V.reduce_f32_emulated(slabs[::-1], bias, res))
    assert not np.array_equal(want, (V.reduce_f32_emulated(slabs, None, res) + bias).astype(np.float32))
    f64 = slabs.astype(np.float64).sum(0) + bias + res
    mag = np.abs(slabs.astype(np.float64)).sum(0) + np.abs(bias) + np.abs(res)        # 6 additions, each within u of a partial sum that |terms| bounds
    assert (np.abs(want - f64) <= 6 * V.U * mag).all()
