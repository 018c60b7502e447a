"""The decode kernels' argument heads (csrc/llm_kernels.hip, "Kernel arguments"): the first memory requests of a mat-vec or attention launch are fed by a head of plain
pointers and ints in front of the structs, and the launchers fill that head slot by slot.  These tests are about an argument bound to the wrong slot, not about the
arithmetic: tiny shapes, every prologue kind, every set size, both fat thread counts, and identity (np.array_equal) between launches that reach the same numbers through
different heads -- the fused prologue against the standalone preparation + the prologue-free kernel, the split attention against the unsplit one."""
import numpy as np
import pytest

from test_cpu_matvec_dispatch import FAMILY

pytestmark = pytest.mark.gpu

KS = (256, 768)            # one super-block (most lanes masked) / three
ROWS = (3, 17, 520)        # fewer rows than waves of a workgroup (the clamp), an odd count, more than one workgroup


def _case(t, n_mat, K, rows, seed):
    from minigpt4_cpp_amd import quants as Q
    rng = np.random.default_rng(seed)
    raw = Q.quantize(t, (0.05 * rng.standard_normal((n_mat * rows, K))).astype(np.float32))
    x = (2.0 * rng.standard_normal(K)).astype(np.float32)
    x2 = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32)        # the norm weight / the second factor: a swap with x shows
    res = rng.standard_normal(n_mat * rows).astype(np.float32)
    return raw, x, x2, res


@pytest.mark.parametrize("wtype", list(FAMILY))
def test_fused_prologue_equals_standalone_preparation_and_prologue_free_launch(gpu_lib, wtype):
    """prep 1 (rms), 2 (plain), 3 (silu) x 1, 2, 3 matrices x residual or none x K x rows; epi 0 launches 512-thread workgroups, epi 2 (the oracle-order forms of the
    k-quants, no SiLU prologue) 768-thread ones.  Shapes the hook refuses (rc 4) are left out and counted: under one in ten."""
    from minigpt4_cpp_amd import quants as Q
    t = Q.NAME_TO_TYPE[wtype]
    tried = refused = 0
    for epi in (0, 2) if wtype in ("q4_k", "q5_k", "q6_k") else (0,):
        for prep in (1, 2, 3) if epi == 0 else (1, 2):
            for n_mat in (1, 2, 3):
                for K in KS:
                    for rows in ROWS:
                        raw, x, x2, res = _case(t, n_mat, K, rows, 1000 * K + 10 * rows + n_mat)
                        for residual in (None, res):
                            tried += 1
                            kw = dict(prep=prep, epi=epi, residual=residual)
                            try:
                                fused = gpu_lib.amd_test_matvec(t, raw, n_mat, K, rows, x, None if prep == 2 else x2, fuse=True, **kw)
                            except RuntimeError as e:
                                assert "rc=4" in str(e), e
                                refused += 1
                                continue
                            alone = gpu_lib.amd_test_matvec(t, raw, n_mat, K, rows, x, None if prep == 2 else x2, fuse=False, **kw)
                            tag = (wtype, epi, prep, n_mat, K, rows, residual is not None)
                            assert fused.shape == (n_mat, rows) and np.isfinite(fused).all() and np.isfinite(alone).all(), tag
                            assert np.abs(alone).max() > 0, tag
                            assert np.array_equal(fused, alone), (tag, float(np.abs(fused - alone).max()))
    print(f"{wtype}: {tried} launch pairs, {refused} refused by the hook")
    assert refused * 10 < tried, (wtype, tried, refused)


@pytest.mark.parametrize("t1", ["q4_k", "q5_k"])
def test_mixed_launch_sets_of_different_row_counts(gpu_lib, t1):
    """wq|wk (two matrices) + a Q6_K wv (one) in one launch: set 1 has twice the rows of set 2, so swapped group or wave counts leave rows unwritten (the hook fills
    the outputs with NaN patterns first) or wrong.  Fused against standalone preparation, and each set against a launch of its own."""
    from minigpt4_cpp_amd import quants as Q
    ta, tb = Q.NAME_TO_TYPE[t1], Q.NAME_TO_TYPE["q6_k"]
    for K in KS:
        for rows in ROWS:
            ra, x, x2, _ = _case(ta, 2, K, rows, 77 * K + rows)
            rb = _case(tb, 1, K, rows, 78 * K + rows)[0]
            tag = (t1, K, rows)
            fused = gpu_lib.amd_test_matvec(ta, ra, 2, K, rows, x, x2, prep=1, fuse=True, type2=tb, raw2=rb)
            alone = gpu_lib.amd_test_matvec(ta, ra, 2, K, rows, x, x2, prep=1, fuse=False, type2=tb, raw2=rb)
            assert fused.shape == (3, rows) and np.isfinite(fused).all(), tag
            assert np.array_equal(fused, alone), tag
            own_a = gpu_lib.amd_test_matvec(ta, ra, 2, K, rows, x, x2, prep=1, fuse=True)
            own_b = gpu_lib.amd_test_matvec(tb, rb, 1, K, rows, x, x2, prep=1, fuse=True)
            assert np.array_equal(fused[:2], own_a) and np.array_equal(fused[2:], own_b), tag


# ---------------------------------------------------------------------------------------------------------------- attention
HD, N_HEAD, N_CTX = 128, 3, 64
POSITIONS = (0, 1, 7, 8, 9)       # only the own key / one cached key / around the 8-key padding of the score row
_ATT = {}


def _attn_inputs():
    if "in" not in _ATT:
        rng = np.random.default_rng(515)
        E = N_HEAD * HD
        q, k = (rng.standard_normal((1, E)).astype(np.float32) for _ in range(2))
        v = (0.5 + rng.standard_normal((1, E)) * np.linspace(0.5, 2.0, E)).astype(np.float32)       # a mean: a probability on the wrong key shows
        kc = rng.standard_normal((1, N_CTX, E)).astype(np.float16).view(np.uint16)
        vc = (0.5 + rng.standard_normal((1, N_CTX, E))).astype(np.float16).view(np.uint16)
        for a in (q, k, v, kc, vc):
            a.setflags(write=False)
        _ATT["in"] = (q, k, v, kc, vc)
    return _ATT["in"]


def _rope_tables():
    """the launchers' tables: theta = pos * 10000^(-2 i / hd), advanced in fp32"""
    P = HD // 2
    c, s = np.empty((N_CTX, P), np.float32), np.empty((N_CTX, P), np.float32)
    scale = np.float32(np.power(np.float32(10000.0), np.float32(-2.0 / HD)))
    for p in range(N_CTX):
        theta = np.float32(p)
        for i in range(P):
            c[p, i], s[p, i] = np.cos(theta), np.sin(theta)
            theta = np.float32(theta * scale)
    return c, s


def _attn_f64(pos):
    """(a) float64 softmax attention over the fp16 keys / values the kernel sees (cached rows below pos, then the rotated fp16 own row); (b) the same with the kernel's
    rounding points: the exponential from the fp16 table on the fp16-rounded s - max, p = fp16(e * float32(1 / sum)).  Also the appended key / value rows."""
    q, k, v, kc, vc = _attn_inputs()
    if "tab" not in _ATT:
        _ATT["tab"] = _rope_tables()
        h = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            _ATT["exp"] = np.exp(h).astype(np.float16).astype(np.float64)
    c, s = _ATT["tab"]
    etab = _ATT["exp"]

    def rot(x):
        x = x.reshape(N_HEAD, HD // 2, 2)
        return np.stack([x[..., 0] * c[pos] - x[..., 1] * s[pos], x[..., 0] * s[pos] + x[..., 1] * c[pos]], axis=-1).astype(np.float16).reshape(N_HEAD, HD)

    qr, kr, vr = rot(q[0]), rot(k[0]), v[0].astype(np.float16).reshape(N_HEAD, HD)
    a, b = np.empty((N_HEAD, HD)), np.empty((N_HEAD, HD))
    for h in range(N_HEAD):
        cs = slice(h * HD, (h + 1) * HD)
        K = np.concatenate([kc[0, :pos, cs].view(np.float16), kr[h:h + 1]]).astype(np.float64)
        V = np.concatenate([vc[0, :pos, cs].view(np.float16), vr[h:h + 1]]).astype(np.float64)
        sc = (K @ qr[h].astype(np.float64)) / np.sqrt(float(HD))
        d = sc - sc.max()
        pa = np.exp(d)
        a[h] = (pa / pa.sum()) @ V
        e = etab[d.astype(np.float32).astype(np.float16).view(np.uint16)]
        inv = np.float32(1.0 / e.sum())
        p = (e.astype(np.float32) * inv).astype(np.float16).astype(np.float64)
        b[h] = p @ V
    return a.reshape(-1), b.reshape(-1), kr.reshape(-1), vr.reshape(-1)


def test_attention_head_at_the_first_positions(gpu_lib):
    """HD 128, one row, positions 0, 1, 7, 8, 9, VS 1 / 2 / 4.  `out` and the appended cache rows of the split launches equal the unsplit launch's bit for bit; the
    unsplit launch meets the float64 reference at the bar of the other attention tests -- twice the noise of the reference's own table arithmetic, |a - b|, here taken
    over the five positions together (a position with one or two keys has next to none of its own; position 0 alone must be exact: p = 1).  The appended key row is
    the rotated row within one fp16 step (the fp32 rotation can round the other way), the appended value row is exact.  A q / k / v / table / cache pointer in the
    wrong slot is orders of magnitude above any of these."""
    q, k, v, kc, vc = _attn_inputs()
    E = N_HEAD * HD
    refs = {pos: _attn_f64(pos) for pos in POSITIONS}
    bar = 2.0 * max(float(np.abs(r[0] - r[1]).max()) for r in refs.values())
    for pos in POSITIONS:
        a, b, kr, vr = refs[pos]
        base = None
        for vs in (1, 2, 4):
            out, kc2, vc2 = gpu_lib.amd_test_attn_vsplit(0, vs, q, k, v, kc, vc, N_HEAD, [0], [pos], computed_exp=False)
            if vs == 1:
                base = (out, kc2, vc2)
                err = float(np.abs(out[0].astype(np.float64) - b).max())
                print(f"pos {pos}: max|got - b| = {err:.3e}, bar = {bar:.3e}, max|b| = {np.abs(b).max():.3e}")
                assert np.isfinite(out).all()
                assert err <= (0.0 if pos == 0 else bar), (pos, err, bar)
                got_k = kc2[0, pos].view(np.float16).astype(np.float64)
                pair = np.abs(k[0].astype(np.float64)).reshape(-1, 2).sum(axis=1).repeat(2)
                assert (np.abs(got_k - kr.astype(np.float64)) <= 2.0 ** -10 * pair).all(), pos
                assert np.array_equal(vc2[0, pos], vr.view(np.uint16)), pos
                keep = np.arange(N_CTX) != pos
                assert np.array_equal(kc2[0, keep], kc[0, keep]) and np.array_equal(vc2[0, keep], vc[0, keep]), pos
            else:
                assert np.array_equal(out, base[0]), (pos, vs, float(np.abs(out - base[0]).max()))
                assert np.array_equal(kc2, base[1]) and np.array_equal(vc2, base[2]), (pos, vs)
    assert E == q.shape[1]
