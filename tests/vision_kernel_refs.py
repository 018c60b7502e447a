"""References for the image encoder's LayerNorm / slab-reduce kernels (csrc/vision_kernels.hip: k_layernorm, k_splitk_reduce_ln), shared by
tests/test_cpu_vision_kernel_refs.py (no GPU: the references checked against each other) and tests/test_gpu_vision_kernels.py (the kernels checked against them).

  ln_f64               plain float64 LayerNorm (eps 1e-5), also returning the row's mean and s = sqrt(variance + eps)
  ln_f32_emulated      k_layernorm statement by statement in np.float32 (sums in float64, mean and variance rounded to fp32)
  reduce_f32_emulated  k_splitk_reduce_ln's per-element chain: a = slab0; a = a + slab_z; v = bias + a; v = residual + v
  ln_bound             the error bound of the fp32 LayerNorm against ln_f64 (derivation at the function)
  row_families / ln_params   the input rows and weights both test files draw
"""
import numpy as np

F = np.float32
EPS = 1e-5
U = 2.0 ** -24                                   # unit roundoff of fp32


def ln_f64(x, w, b=None, eps=EPS):
    """-> (out, mu, s): float64 LayerNorm of the rows of x; mu / s = the row's mean and sqrt(variance + eps), shape [rows, 1]."""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    s = np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps)
    out = (x - mu) / s * np.asarray(w, np.float64)
    if b is not None:
        out = out + np.asarray(b, np.float64)
    return out, mu, s


def _sum64(v, sequential):
    """Sum of the rows of v in float64: ONE accumulator in element order (np.cumsum adds left to right; np.sum is pairwise), or any float64 order."""
    v = v.astype(np.float64)
    return np.cumsum(v, axis=-1)[..., -1:] if sequential else v.sum(-1, keepdims=True)


def ln_f32_emulated(x, w, b=None, sequential=False, eps=F(1e-5)):
    """k_layernorm in np.float32, one statement per line of the kernel.  sequential: the two sums with one float64 accumulator in element order (the kernel's
    sequential_sums form, ggml_norm's loops) -- then the result is the kernel's BIT FOR BIT; otherwise the float64 sums are in numpy's order (the kernel's is a tree over
    lanes and waves: both are float64 sums of the same terms, they differ by ~1e-16 relative before the rounding to fp32)."""
    x = np.asarray(x, F)
    n = x.shape[-1]
    mean = (_sum64(x, sequential) / np.float64(n)).astype(F)              # mean = (float)(sum / (double)n)
    d = x - mean                                                          # v = x - mean                     (fp32)
    sq = d * d                                                            # v * v                            (fp32)
    variance = (_sum64(sq, sequential) / np.float64(n)).astype(F)         # variance = (float)(sum2 / (double)n)
    scale = F(1.0) / np.sqrt(variance + F(eps), dtype=F)                  # 1.0f / sqrtf(variance + 1e-5f)
    v = d * scale                                                         # (x - mean) * scale
    v = np.asarray(w, F) * v                                              # w * v
    if b is not None:
        v = v + np.asarray(b, F)                                          # v + b
    assert v.dtype == F
    return v


def reduce_f32_emulated(slabs, bias=None, residual=None):
    """slabs [n_slabs][rows][n] fp32 -> x [rows][n]: the kernel's additions in the kernel's order, each rounded to fp32."""
    slabs = np.asarray(slabs, F)
    a = slabs[0].copy()
    for z in range(1, slabs.shape[0]):
        a = a + slabs[z]
    v = a
    if bias is not None:
        v = np.asarray(bias, F) + a
    if residual is not None:
        v = np.asarray(residual, F) + v
    assert v.dtype == F
    return v


def ln_bound(x, w, b=None, margin=2.0):
    """Per-element bound on |fp32 LayerNorm - ln_f64|, u = 2^-24:

        bound_i = margin * u * ( |w_i| * ( |mu| / s + 10 * |xhat_i| ) + |want_i| ),   xhat_i = (x_i - mu) / s,   margin = 2

    The fp32 mean is off by <= u |mu|, which moves every normalised value by u |mu| / s; x - mean adds u |x - mean|; the mean's error enters the variance only at second
    order (sum(x - mu) = 0), so the variance carries ~4u (the subtraction twice, the square, its own rounding) and 1 / sqrtf(variance + eps) ~5u (half of 4u, the add, the
    square root, the division); the two multiplies and the add contribute 3u, the last one on |want_i|.  ~9u on the normalised value, rounded up to 10."""
    want, mu, s = ln_f64(x, w, b)
    xhat = (np.asarray(x, np.float64) - mu) / s
    return margin * U * (np.abs(np.asarray(w, np.float64)) * (np.abs(mu) / s + 10.0 * np.abs(xhat)) + np.abs(want))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "residual_stream", "constant", "zero", "outlier")


def row_families(rng, n):
    """One row of n values per family, in FAMILIES' order -> fp32 [5][n]: standard normal; mean 40, spread 1 (a residual stream: the mean is large against the spread);
    a constant row and an all-zero row (variance 0: eps decides); one +-300 outlier in an otherwise small row."""
    rows = np.empty((len(FAMILIES), n), F)
    rows[0] = rng.standard_normal(n)
    rows[1] = 40.0 + rng.standard_normal(n)
    rows[2] = F(rng.uniform(-3.0, 3.0))
    rows[3] = 0.0
    rows[4] = 0.01 * rng.standard_normal(n)
    rows[4, rng.integers(0, n)] = 300.0 * rng.choice([-1.0, 1.0])
    return rows


def ln_params(rng, n):
    """w about 1 +- 0.2 with a few negative entries, b about +-1."""
    w = (1.0 + 0.2 * rng.standard_normal(n)).astype(F)
    w[rng.integers(0, n, max(1, n // 64))] *= F(-1.0)
    b = (rng.choice([-1.0, 1.0], n) * (1.0 + 0.1 * rng.standard_normal(n))).astype(F)
    return w, b


def ln_case(n):
    """The LayerNorm input of row length n both test files use: (x fp32 [5][n] = row_families, w, b)."""
    rng = np.random.default_rng(1000 + n)
    x = row_families(rng, n)
    w, b = ln_params(rng, n)
    return x, w, b


def reduce_case(rng, n_slabs, rows, n):
    """-> (slabs fp32 [n_slabs][rows][n], bias [n], residual [rows][n]).  Every slab is a normal of its OWN magnitude (0.01 .. 10), so that adding the slabs in another order,
    or bias / residual at another point of the chain, rounds differently; the rows of the residual are families of the list above (which ones changes from draw to draw), so the LayerNorm that follows sees them."""
    slabs = np.stack([(10.0 ** rng.uniform(-2.0, 1.0)) * rng.standard_normal((rows, n)) for _ in range(n_slabs)]).astype(F)
    bias = rng.standard_normal(n).astype(F)
    fam = row_families(rng, n)
    residual = fam[np.array([1, 0, 4, 2, 3])[(np.arange(rows) + rng.integers(0, 5)) % 5]]
    return slabs, bias, residual


# ---- deliberately wrong LayerNorms: what the bound has to catch (tests/test_cpu_vision_kernel_refs.py) -------------------------------------------------------------------
def ln_mean_in_fp32(x, w, b=None):
    """the mean summed pairwise in fp32 instead of float64"""
    x = np.asarray(x, F)
    mean = (x.sum(-1, keepdims=True, dtype=F) / F(x.shape[-1])).astype(F)
    d = x - mean
    variance = (_sum64(d * d, False) / np.float64(x.shape[-1])).astype(F)
    v = np.asarray(w, F) * (d * (F(1.0) / np.sqrt(variance + F(1e-5), dtype=F)))
    return v if b is None else v + np.asarray(b, F)


def ln_variance_without_mean(x, w, b=None):
    """variance = E[x^2] (the mean not subtracted before squaring)"""
    x = np.asarray(x, F)
    mean = (_sum64(x, False) / np.float64(x.shape[-1])).astype(F)
    variance = (_sum64(x * x, False) / np.float64(x.shape[-1])).astype(F)
    v = np.asarray(w, F) * ((x - mean) * (F(1.0) / np.sqrt(variance + F(1e-5), dtype=F)))
    return v if b is None else v + np.asarray(b, F)


def ln_eps_1e6(x, w, b=None):
    return ln_f32_emulated(x, w, b, eps=F(1e-6))


PERTURBED = {"mean_in_fp32": ln_mean_in_fp32, "variance_without_mean": ln_variance_without_mean, "eps_1e-6": ln_eps_1e6}
