"""The decode mat-vec's launchers against the predicates the engine asks first, at the edges of every instantiated unit count, and the multi-row kernel (k_matvec_tn)
preparing its own rows -- the in-launch preparations the whole-engine tests reach only through complete decode steps."""
import numpy as np
import pytest

from test_cpu_matvec_dispatch import FAMILY, cases
from test_gpu_parity import _prepared_row, _silu_table

pytestmark = pytest.mark.gpu

# the K that breaks a type's divisibility rule cannot be launched through the hook: it is no whole number of the type's blocks (the hook's argument check refuses it before
# a launcher is asked), or, for F16, the launchers themselves do not look at it -- only the predicate, which the engine asks first, does (test_cpu_matvec_dispatch)
EDGES = [(t, K) for t in ("q4_0", "q4_k", "q6_k", "q8_0", "f16") for K, launchable in cases(t) if launchable]


@pytest.mark.parametrize("wtype,K", EDGES)
def test_fused_prologue_launches_exactly_where_the_predicate_says(gpu_lib, wtype, K):
    """prep 1 / 2 / 3 fused into the launch, 70 weight rows: predicate yes -> the launch exists and meets the 2e-5-of-row-maximum bar of every mat-vec kernel against the
    oracle on the identically prepared row; predicate no -> the launcher refuses (the hook's return code 4), nothing is launched."""
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    rows = 70
    rng = np.random.default_rng(K * 3 + sum(map(ord, wtype)))
    raw = Q.quantize(t, (0.03 * rng.standard_normal((rows, K))).astype(np.float32))
    yes = gpu_lib.amd_test_matvec_predicates(t, K)[0]
    assert yes == (K <= FAMILY[wtype][1][-1] * 64 * FAMILY[wtype][0])
    for prep in (1, 2, 3):
        x = (rng.standard_normal(K) * (3.0 if prep == 3 else 1.0)).astype(np.float32)
        x2 = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32) if prep != 2 else None
        if not yes:
            with pytest.raises(RuntimeError, match="rc=4"):
                gpu_lib.amd_test_matvec(t, raw, 1, K, rows, x, x2, prep=prep, fuse=True)
            continue
        got = gpu_lib.amd_test_matvec(t, raw, 1, K, rows, x, x2, prep=prep, fuse=True).reshape(-1)
        want = R.mul_mat(t, raw, K, rows, _prepared_row(prep, x, x2, _silu_table())[None, :])[0]
        assert np.isfinite(got).all()
        assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max(), (wtype, K, prep, float(np.abs(got - want).max() / np.abs(want).max()))


@pytest.mark.parametrize("wtype", ["q4_0", "q4_k", "q5_k", "q6_k"])
@pytest.mark.parametrize("K", [512, 4096, 5120])           # 1, 2, 3 units per lane (5120: ragged)
@pytest.mark.parametrize("N,n_mat", [(1, 1), (3, 3), (4, 1)])
def test_multi_row_matvec_prepares_its_own_rows(gpu_lib, wtype, K, N, n_mat):
    """k_matvec_tn with the rows handed over as fp32 (PRO = 1: rms_norm(x_t) * w, PRO = 2: as they are) against the oracle's mul_mat on the rows prepared the way ggml
    prepares them, at the 2e-5 bar; 2300 rows so that waves pipeline more than one group.  One row, norm form: the single-row kernel's prologue does the same arithmetic
    on the same weights -> bit-identical to it."""
    import refcpu as R
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    rows = 2300
    rng = np.random.default_rng(K * 17 + N * 5 + n_mat + sum(map(ord, wtype)))
    raw = Q.quantize(t, (0.03 * rng.standard_normal((n_mat * rows, K))).astype(np.float32))
    x = rng.standard_normal((N, K)).astype(np.float32)
    x[0, :256] = 0.0                                        # an all-zero activation block
    if N > 1:
        x[1] *= 37.0                                        # rows of very different magnitude: per-row scales
    nw = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32)
    for w in (nw, None):
        got = gpu_lib.amd_test_matvec_rows(t, raw, n_mat, K, rows, x, rms_w=w, prepare=True)
        prepared = x if w is None else np.stack([_prepared_row(1, x[i], w, None) for i in range(N)])
        want = R.mul_mat(t, raw, K, n_mat * rows, prepared).reshape(N, n_mat, rows).transpose(1, 0, 2)
        scale = np.abs(want).max(axis=2, keepdims=True)
        assert got.shape == want.shape and np.isfinite(got).all()
        assert (np.abs(got - want) <= 2e-5 * scale).all(), (wtype, K, N, n_mat, w is not None, float((np.abs(got - want) / scale).max()))
        if N == 1 and w is not None:
            one = gpu_lib.amd_test_matvec(t, raw, n_mat, K, rows, x[0], w, prep=1, fuse=True)
            assert np.array_equal(got[:, 0, :], one), (wtype, K, n_mat)
