"""When the decode mat-vec's prologue forms issue their weight loads (csrc/llm_kernels.hip: matvec_run).

Prefetch depths 2 and 3 -- a second and a third row group requested before the row preparation -- were built, measured and lost at every launch site
(profiles/r13_matvec_prefetch_depth.log), so their kernels are gone again.  What stayed is the issue barrier (IB): a data-free s_barrier between the prologue's row loads and
its first weight requests.  It moves only the moment at which loads are issued, so every output must equal the barrier-free launch's BIT FOR BIT (np.array_equal, no
tolerance), nothing may be stored behind the outputs, and a whole decode step must give the same ids and logits whatever MINIGPT4_MV_IB says.

The grid is the one the depths were tested on: row counts that give waves 0, 1, 2, 3 and 4 row groups (wave w owns groups w, w + n_waves, ...; n_waves from the hook: a wave
without a group still has to reach the barrier), K with one and three units per lane, full and ragged, every prologue / epilogue kind, sets and mixed-type launches.

The barrier forms are built for the k-quants at up to three units per lane (K <= 6144); elsewhere the launch runs the plain form (Q8_0 / F16: their cases here check
exactly that asking for the barrier is harmless)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
POOL_ROWS = 61                                                       # distinct quantised rows, cycled: row r = pool[r % 61] (prime: a wrong row index shows)


def _rows(nw):
    return [1, 7, nw - 1, nw + 1, 5 * nw // 2, 3 * nw + 5]


_pools = {}


def _raw(wtype, rows, K, salt=0):
    """`rows` quantised rows of K weights as file bytes, cycled from a small pool (quantised once per type / K / salt)."""
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    key = (wtype, K, salt)
    if key not in _pools:
        rng = np.random.default_rng(1000 * K + 7 * t + salt)
        _pools[key] = np.ascontiguousarray(Q.quantize(t, (0.05 * rng.standard_normal(POOL_ROWS * K)).astype(np.float32))).view(np.uint8).reshape(POOL_ROWS, -1)
    pool = _pools[key]
    return t, np.ascontiguousarray(pool[np.arange(rows) % POOL_ROWS]).reshape(-1)


def _inputs(K, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(K).astype(np.float32), (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32)


def _check(gpu_lib, **kw):
    base, g0 = gpu_lib.amd_test_matvec_issue(issue_barrier=False, guard=GUARD, **kw)
    assert np.isfinite(base).all() and (g0 == 0xFFFFFFFF).all()
    got, g = gpu_lib.amd_test_matvec_issue(issue_barrier=True, guard=GUARD, **kw)
    assert np.array_equal(got, base), (kw["n_out"], kw["n_in"])
    assert (g == 0xFFFFFFFF).all(), "stored behind the outputs"


@pytest.mark.parametrize("wtype", ["q4_k", "q5_k", "q6_k"])
@pytest.mark.parametrize("K", [256, 2048, 5120])
def test_row_counts(gpu_lib, wtype, K):
    """rms-norm prologue, one matrix, every row count.  K 256 / 2048: one unit per lane (a quarter of the lanes / all of them), two rows per group; 5120: three
    units per lane with 160 of 192 slots used, one row per group."""
    nw = gpu_lib.amd_test_matvec_waves()
    x, w = _inputs(K, K)
    for rows in _rows(nw):
        t, raw = _raw(wtype, rows, K)
        _check(gpu_lib, type1=t, raw1=raw, n1=1, n_in=K, n_out=rows, x=x, x2=w, prep=1)


@pytest.mark.parametrize("wtype", ["q4_k", "q5_k", "q6_k"])
@pytest.mark.parametrize("prep", [1, 2, 3])
@pytest.mark.parametrize("with_res", [False, True])
def test_prologue_kinds_and_residual(gpu_lib, wtype, prep, with_res):
    """rms-norm | plain | silu(a) * b prologue, with and without the residual add, at the two ends of the groups-per-wave range (1 | 2 and 4 | 3) and both group shapes."""
    nw = gpu_lib.amd_test_matvec_waves()
    for K in (256, 5120):
        x, w = _inputs(K, 3 * K + prep)
        for rows in (nw + 1, 3 * nw + 5):
            t, raw = _raw(wtype, rows, K)
            res = np.random.default_rng(rows).standard_normal(rows).astype(np.float32) if with_res else None
            _check(gpu_lib, type1=t, raw1=raw, n1=1, n_in=K, n_out=rows, x=x, x2=None if prep == 2 else w, prep=prep, residual=res)


@pytest.mark.parametrize("wtype", ["q4_k", "q5_k", "q6_k"])
def test_silu_pair_epilogue(gpu_lib, wtype):
    """w1 | w3 as the feed-forward block launches them: two 512 x 5120 matrices, group g = the row pair (w1[g], w3[g]), one output row; and a pair of 2 n_waves + 3 rows
    (waves with 3 and 2 pairs)."""
    nw = gpu_lib.amd_test_matvec_waves()
    K = 5120
    x, w = _inputs(K, 77)
    for rows in (512, 2 * nw + 3):
        t, raw = _raw(wtype, 2 * rows, K, salt=1)
        _check(gpu_lib, type1=t, raw1=raw, n1=2, n_in=K, n_out=rows, x=x, x2=w, prep=1, epi=1)


@pytest.mark.parametrize("wtype", ["q4_k", "q5_k", "q6_k"])
def test_set_of_three(gpu_lib, wtype):
    """wq | wk | wv as one row space: a group's matrix is selected from its row, so the seams (rows_each not a multiple of the wave count) and the clamped over-fetch
    behind the LAST matrix are where a changed issue order could read or store the wrong row.  With a residual per matrix."""
    nw = gpu_lib.amd_test_matvec_waves()
    for K, rows in ((5120, nw // 3 + 5), (5120, nw + 1), (256, 2 * nw // 3 + 1)):
        x, w = _inputs(K, rows)
        t, raw = _raw(wtype, 3 * rows, K, salt=2)
        res = np.random.default_rng(rows).standard_normal(3 * rows).astype(np.float32)
        _check(gpu_lib, type1=t, raw1=raw, n1=3, n_in=K, n_out=rows, x=x, x2=w, prep=1, residual=res)


@pytest.mark.parametrize("t1", ["q5_k", "q4_k"])
def test_mixed_type_launch(gpu_lib, t1):
    """wq | wk (Q5_K / Q4_K) + wv (Q6_K) in one launch, the workgroups split between the halves by bytes.  At 256 workgroups of 8 waves: 800 rows each = 1600 + 800 groups --
    two per wave is the cheapest for the first half and leaves the second half ONE group per wave (both single is 2400 > 2048 waves); 1100 rows: two per wave in both; 37 rows:
    most waves own nothing; 3000 rows: 3 - 5 groups per wave."""
    for K in (5120, 256):
        x, w = _inputs(K, 5)
        for rows in (37, 800, 1100, 3000):
            ta, ra = _raw(t1, 2 * rows, K, salt=3)
            tb, rb = _raw("q6_k", rows, K, salt=4)
            _check(gpu_lib, type1=ta, raw1=ra, n1=2, type2=tb, raw2=rb, n_in=K, n_out=rows, x=x, x2=w, prep=1)


@pytest.mark.parametrize("wtype,K", [("q8_0", 256), ("q8_0", 4096), ("f16", 512), ("f16", 1024)])
def test_types_without_a_barrier_form_run_the_plain_one(gpu_lib, wtype, K):
    """Q8_0 / F16 at K values their narrow forms take: no barrier form is built for them, asking for it runs the plain kernel -- same bits, no refusal."""
    nw = gpu_lib.amd_test_matvec_waves()
    x, w = _inputs(K, 11)
    for rows in (7, nw + 1):
        t, raw = _raw(wtype, rows, K)
        _check(gpu_lib, type1=t, raw1=raw, n1=1, n_in=K, n_out=rows, x=x, x2=w, prep=1)


def test_whole_step_is_bit_identical_with_and_without_the_barrier(gpu_lib, tiny_files):
    """40 greedy steps on the conditioned tiny q5_k_m model in three contexts (MINIGPT4_MV_IB unset = the per-site defaults, 0 = off everywhere, 1 = on everywhere; read per
    engine): the same ids and, at the last step, the same logits bit for bit."""
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    toks = [1] + [int(t) for t in np.random.default_rng(13).integers(3, 512, 19)]
    runs = {}
    for ib in (None, "0", "1"):
        os.environ.pop("MINIGPT4_MV_IB", None)
        if ib is not None:
            os.environ["MINIGPT4_MV_IB"] = ib
        try:
            ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=128, n_batch=32)
        finally:
            os.environ.pop("MINIGPT4_MV_IB", None)
        try:
            gpu_lib.amd_eval_tokens(ctx, toks)
            got = gpu_lib.amd_logits(ctx).copy()
            ids = []
            for _ in range(40):
                ids.append(int(got.argmax()))
                gpu_lib.amd_eval_tokens(ctx, [ids[-1]])
                got = gpu_lib.amd_logits(ctx).copy()
            runs[ib] = (ids, got)
        finally:
            gpu_lib.minigpt4_free(ctx)
    assert len(set(runs["0"][0])) > 4                       # a conversation, not one token repeated
    for ib in (None, "1"):
        assert runs[ib][0] == runs["0"][0]
        assert np.array_equal(runs[ib][1], runs["0"][1])
