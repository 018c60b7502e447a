"""The quantised mat-mul / mat-vec kernels and the embedding gather on arbitrary block bytes against float64 (tests/quant_blocks.py: generators, decoders, the bound).

Every case runs BOTH block generators (uniformly random bytes with finite fp16 fields; constant extreme patterns) against activation rows that quantise exactly, and asserts
per OUTPUT ELEMENT  |got - x . w| <= (n_blocks + 4) * 2^-24 * (|x| . a)  -- ratio <= 1 -- instead of 2e-5 of the row maximum; outputs finite; guards untouched where a hook
has them.  tests/test_cpu_quant_blocks.py holds the oracle to the same inputs (its ratios: <= 0.36) and shows that every mutant decoder leaves the bound on them.
A hook that refuses a shape (4) FAILS the test: the cases are chosen to be supported, a skip would hide a dispatch change.
The largest ratio per kernel family and type goes to conftest.record_observed as quant_blocks/<family>/<type>."""
import numpy as np
import pytest

import quant_blocks as QB
from conftest import record_observed

pytestmark = pytest.mark.gpu
GENS = ("random", "extreme")


def _ids(cases, fmt):
    return [fmt % ((QB.NAMES[c[0]],) + tuple(c[1:])) for c in cases]


def _check(family, t, gen, n_rows_set, K, got, act_index, row_slice=slice(None), residual=None, what=""):
    """got [N][rows] for activation rows act_index against rows row_slice of the weight set (gen, t, n_rows_set, K)"""
    exact, mag = QB.reference(gen, t, n_rows_set, K)
    exact, mag = exact[act_index][:, row_slice], mag[act_index][:, row_slice]
    assert got.shape == exact.shape, (got.shape, exact.shape)
    assert np.isfinite(got).all(), (family, QB.NAMES[t], gen, what)
    r = QB.ratio_of(got, exact, mag, QB.n_blocks(t, K), residual)
    print("quant_blocks/%s/%s %s K%d %s: ratio %.4f" % (family, QB.NAMES[t], gen, K, what, r))
    record_observed("quant_blocks/%s/%s" % (family, QB.NAMES[t]), r)
    return r


def _assert_all(ratios):
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("t,N,K,n_out", QB.MUL_MAT_CASES, ids=_ids(QB.MUL_MAT_CASES, "%s-N%d-K%d-R%d"))
def test_mul_mat_on_arbitrary_blocks(gpu_lib, t, N, K, n_out):
    """k_mul_mat (N < 16) and the prefill dispatch (N >= 16: the int8 / f16 MFMA routes), Q3_K through its load-time conversion"""
    ratios = {}
    for gen in GENS:
        for first in ((0, 3, 6) if N < QB.N_ACT else (0,)):
            idx = QB.rows_index(N, first)
            got = gpu_lib.amd_test_mul_mat(t, QB.blocks(gen, t, n_out, K).reshape(-1), K, n_out, QB.act_rows(t, K, N, first))
            ratios[(gen, first)] = _check("mul_mat", t, gen, n_out, K, got, idx, what="N%d first%d" % (N, first))
    _assert_all(ratios)


@pytest.mark.parametrize("t", QB.MMQ2_TYPES, ids=lambda t: QB.NAMES[t])
@pytest.mark.parametrize("shape", QB.MMQ2_SHAPES, ids=lambda c: "N%d_K%d_R%d_m%d_ks%d_res%d" % c)
def test_mmq2_on_arbitrary_blocks(gpu_lib, t, shape):
    """generation 2 (k_mmq2_*): one partial tile, two tiles / two matrices / ragged rows, a forced K split with a residual of small integers"""
    N, K, n_out, n_mat, ks, with_res = shape
    idx = QB.rows_index(N)
    res = np.random.default_rng(N + K).integers(-3, 4, (n_mat, N, n_out)).astype(np.float32) if with_res else None
    ratios = {}
    for gen in GENS:
        got = gpu_lib.amd_test_mmq2(t, QB.blocks(gen, t, n_mat * n_out, K).reshape(-1), n_mat, K, n_out, QB.act_rows(t, K, N), residual=res, ks=ks, generation=2)
        for m in range(n_mat):
            ratios[(gen, m)] = _check("mmq2", t, gen, n_mat * n_out, K, got[m], idx, slice(m * n_out, (m + 1) * n_out), None if res is None else res[m].astype(np.float64), "mat%d" % m)
    _assert_all(ratios)


@pytest.mark.parametrize("t,K,rows", QB.MATVEC_SHAPES, ids=_ids(QB.MATVEC_SHAPES, "%s-K%d-R%d"))
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("n_mat", [1, 3])
def test_decode_matvec_on_arbitrary_blocks(gpu_lib, t, K, rows, fuse, n_mat):
    """k_matvec_v2 with the plain-row preparation (prep 2) stand-alone and in the prologue -- the in-prologue quantiser is exact on these rows too"""
    ratios = {}
    for gen in GENS:
        raw = QB.blocks(gen, t, 3 * rows, K)[:n_mat * rows]
        for a in range(6):
            got = gpu_lib.amd_test_matvec(t, raw.reshape(-1), n_mat, K, rows, QB.activation_rows(t, K)[a], prep=2, fuse=fuse).reshape(1, n_mat * rows)
            ratios[(gen, a)] = _check("matvec", t, gen, 3 * rows, K, got, [a], slice(0, n_mat * rows), what="row%d fuse%d m%d" % (a, fuse, n_mat))
    _assert_all(ratios)


@pytest.mark.parametrize("ta,K,rows", QB.MATVEC_MIX_SHAPES, ids=_ids(QB.MATVEC_MIX_SHAPES, "%s-K%d-R%d"))
def test_decode_matvec_mixed_launch_on_arbitrary_blocks(gpu_lib, ta, K, rows):
    """k_matvec_mix: two Q4_K / Q5_K matrices and a Q6_K third in one launch (its prologue has the rms form only, which is not exact: the rows are prepared stand-alone)"""
    ratios = {}
    for gen in GENS:
        ra, rb = QB.blocks(gen, ta, 3 * rows, K)[:2 * rows], QB.blocks(gen, QB.Q6_K, 3 * rows, K)[:rows]
        for a in range(6):
            got = gpu_lib.amd_test_matvec(ta, ra.reshape(-1), 2, K, rows, QB.activation_rows(ta, K)[a], prep=2, fuse=False, type2=QB.Q6_K, raw2=rb.reshape(-1)).reshape(1, 3 * rows)
            ratios[(gen, a, "a")] = _check("matvec_mix", ta, gen, 3 * rows, K, got[:, :2 * rows], [a], slice(0, 2 * rows), what="row%d" % a)
            ratios[(gen, a, "b")] = _check("matvec_mix", QB.Q6_K, gen, 3 * rows, K, got[:, 2 * rows:], [a], slice(0, rows), what="row%d" % a)
    _assert_all(ratios)


@pytest.mark.parametrize("t,K,rows", QB.ROWS_SHAPES, ids=_ids(QB.ROWS_SHAPES, "%s-K%d-R%d"))
@pytest.mark.parametrize("N", [1, 3, 4])
@pytest.mark.parametrize("n_mat", [1, 3])
def test_multi_row_matvec_on_arbitrary_blocks(gpu_lib, t, K, rows, N, n_mat):
    """k_matvec_tn: 1, 3 and 4 rows (TN 2, 3, 4) against one and three matrices"""
    ratios = {}
    for gen in GENS:
        raw = QB.blocks(gen, t, 3 * rows, K)[:n_mat * rows]
        for first in (0, 3) if N > 1 else range(6):
            idx = QB.rows_index(N, first)
            got = gpu_lib.amd_test_matvec_rows(t, raw.reshape(-1), n_mat, K, rows, QB.act_rows(t, K, N, first))
            for m in range(n_mat):
                ratios[(gen, first, m)] = _check("matvec_rows", t, gen, 3 * rows, K, got[m], idx, slice(m * rows, (m + 1) * rows), what="N%d first%d mat%d" % (N, first, m))
    _assert_all(ratios)


@pytest.mark.parametrize("ta,K,rows", QB.MATVEC_MIX_SHAPES, ids=_ids(QB.MATVEC_MIX_SHAPES, "%s-K%d-R%d"))
@pytest.mark.parametrize("N", [1, 3, 4])
def test_multi_row_mixed_launch_on_arbitrary_blocks(gpu_lib, ta, K, rows, N):
    """k_matvec_tn_mix: two Q4_K / Q5_K matrices and a Q6_K third against 1, 3 and 4 rows in one launch; the guard row behind the outputs keeps its fill"""
    ratios = {}
    for gen in GENS:
        ra, rb = QB.blocks(gen, ta, 3 * rows, K)[:2 * rows], QB.blocks(gen, QB.Q6_K, 3 * rows, K)[:rows]
        for first in (0, 3) if N > 1 else range(6):
            idx = QB.rows_index(N, first)
            got, guard = gpu_lib.amd_test_matvec_rows_mixed(ta, ra.reshape(-1), 2, QB.Q6_K, rb.reshape(-1), 1, K, rows, QB.act_rows(ta, K, N, first))
            assert (guard == 0xFFFFFFFF).all(), (gen, first, "guard row written")
            for m in range(2):
                ratios[(gen, first, m)] = _check("matvec_rows_mix", ta, gen, 3 * rows, K, got[m], idx, slice(m * rows, (m + 1) * rows), what="N%d first%d mat%d" % (N, first, m))
            ratios[(gen, first, 2)] = _check("matvec_rows_mix", QB.Q6_K, gen, 3 * rows, K, got[2], idx, slice(0, rows), what="N%d first%d" % (N, first))
    _assert_all(ratios)


@pytest.mark.parametrize("t,K,rows", QB.RI_SHAPES, ids=_ids(QB.RI_SHAPES, "%s-K%d-R%d"))
@pytest.mark.parametrize("N", [1, 4])
def test_row_interleaved_matvec_on_arbitrary_blocks(gpu_lib, t, K, rows, N):
    """k_ri_build + k_matvec_ri (rms_w NULL: rows prepared in front): the 8-wave form, and the K split over workgroups at (5120, 128) and (4096, 64)"""
    ratios = {}
    for gen in GENS:
        for n_mat in (1, 3):
            raw = QB.blocks(gen, t, 3 * rows, K)[:n_mat * rows]
            for first in (0, 4) if N > 1 else (0, 1, 2, 4):
                idx = QB.rows_index(N, first)
                got = gpu_lib.amd_test_matvec_ri(t, raw.reshape(-1), n_mat, K, rows, QB.act_rows(t, K, N, first))
                for m in range(n_mat):
                    ratios[(gen, n_mat, first, m)] = _check("matvec_ri", t, gen, 3 * rows, K, got[m], idx, slice(m * rows, (m + 1) * rows), what="N%d first%d m%d/%d" % (N, first, m, n_mat))
    _assert_all(ratios)


@pytest.mark.parametrize("ta,K,rows", QB.RI_MIX_SHAPES, ids=_ids(QB.RI_MIX_SHAPES, "%s-K%d-R%d"))
@pytest.mark.parametrize("N", [1, 4])
def test_row_interleaved_mixed_launch_on_arbitrary_blocks(gpu_lib, ta, K, rows, N):
    """k_matvec_ri_mix: two Q4_K / Q5_K matrices + one Q6_K"""
    ratios = {}
    for gen in GENS:
        ra, rb = QB.blocks(gen, ta, 3 * rows, K)[:2 * rows], QB.blocks(gen, QB.Q6_K, 3 * rows, K)[:rows]
        for first in (0, 4) if N > 1 else (0, 1, 2, 4):
            idx = QB.rows_index(N, first)
            got = gpu_lib.amd_test_matvec_ri_mixed(ta, ra.reshape(-1), 2, QB.Q6_K, rb.reshape(-1), 1, K, rows, QB.act_rows(ta, K, N, first))
            for m in range(2):
                ratios[(gen, first, m)] = _check("matvec_ri_mix", ta, gen, 3 * rows, K, got[m], idx, slice(m * rows, (m + 1) * rows), what="N%d first%d mat%d" % (N, first, m))
            ratios[(gen, first, 2)] = _check("matvec_ri_mix", QB.Q6_K, gen, 3 * rows, K, got[2], idx, slice(0, rows), what="N%d first%d" % (N, first))
    _assert_all(ratios)


@pytest.mark.parametrize("t,K", QB.GET_ROWS_CASES, ids=_ids(QB.GET_ROWS_CASES, "%s-K%d"))
def test_get_rows_on_arbitrary_blocks(gpu_lib, t, K):
    """k_get_rows / dequant_elem, the second per-element decoder: every gathered element equals the float64 decoder within one fp32 ulp of a (the one rounding of a two-term
    form), exactly for the one-term types; the row of token -1 and the guard row keep their fill"""
    n, tokens = QB.GET_ROWS_TABLE, QB.GET_ROWS_TOKENS
    for gen in GENS:
        raw = QB.blocks(gen, t, n, K)
        out = gpu_lib.amd_test_get_rows(t, raw.reshape(-1), n, K, tokens)
        assert out.shape == (len(tokens) + 1, K)
        w, a = QB.decode(t, raw, n * K)
        w, a = w.reshape(n, K), a.reshape(n, K)
        worst = 0.0
        for i, tok in enumerate(tokens):
            if tok < 0:
                assert (out[i].view(np.uint32) == 0xFFFFFFFF).all(), (gen, "the row of token -1 was written")
                continue
            assert np.isfinite(out[i]).all()
            err = np.abs(out[i].astype(np.float64) - w[tok])
            if t in QB.TWO_TERM:
                ulp = np.spacing(a[tok].astype(np.float32)).astype(np.float64)
                assert (err <= ulp).all(), (gen, QB.NAMES[t], K, i, int(np.argmax(err / ulp)))
                worst = max(worst, float((err / ulp).max()))
            else:
                assert (err == 0).all(), (gen, QB.NAMES[t], K, i, int(np.argmax(err)))
        assert (out[len(tokens)].view(np.uint32) == 0xFFFFFFFF).all(), (gen, "guard row written")
        record_observed("quant_blocks/get_rows/%s" % QB.NAMES[t], worst)          # in ulps of a (0 for the one-term types)
