"""tests/act_ref.py held to the oracle, no GPU: (1) its quantisers equal refcpu.quantize_row bit for bit on every family and shape -- two independent statements of ggml's
rule agree; (2) no row of the committed inputs is ambiguous for the rms mean, so tests/test_gpu_act_prepare.py may demand exact bits on every row; (3) every family sits in
a first block, a last block and a block of the second loop pass; (4) each named wrong rule changes the plane it governs on the committed inputs -- the inputs reach the
edges; (5) the four hooks refuse bad arguments with 1, with or without a device."""
import ctypes

import numpy as np
import pytest

import act_ref as A
import refcpu as R
from minigpt4_cpp_amd import quants as Q

SHAPES = [(K, N) for K in A.K_32 for N in A.NS]
_ids = lambda v: "K%d_N%d" % v if isinstance(v, tuple) else str(v)   # noqa: E731


def _table():
    return R.table(1)


def _value_sets(K, N):
    """the prepared values of every GPU `prepare` case at (K, N): the plain rows, the normed rows, silu(a) * b"""
    x = A.rows(K, N)[0]
    a, b = A.silu_operands(K, N)
    return {"plain": x, "rms": A.rms_values(x, A.norm_weight(K)), "silu": A.silu_values(a, b, _table())}


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_quantisers_equal_the_oracles_quantize_row(shape):
    K, N = shape
    for name, v in _value_sets(K, N).items():
        for r in range(N):
            row = v[r]
            if K % 256 == 0:
                mine = A.q8k_planes(row[None, :])
                q = R.quantize_row(Q.GGML_Q8_K, row).reshape(K // 256, 292)
                assert np.array_equal(q[:, 0:4].copy().view(np.uint32)[:, 0], mine["dk"][0].view(np.uint32)), (name, r)
                assert np.array_equal(q[:, 4:260].copy().view(np.int8).reshape(-1), mine["q8k"][0]), (name, r)
                assert np.array_equal(q[:, 260:292].copy().view(np.int16).reshape(-1), mine["bsk"][0]), (name, r)
                s32 = mine["q8k"][0].astype(np.int64).reshape(-1, 8, 32).sum(axis=2)                    # the digit planes restate the per-32 sums
                assert np.array_equal(128 * mine["bsq"][0][:, 8:].astype(np.int64) + mine["bsq"][0][:, :8], s32) and (mine["bsq"][0][:, :8] >= 0).all()
                assert np.array_equal(mine["bs16"][0].view(np.float16).astype(np.int64), mine["bsq"][0])
            mine = A.q80_planes(row[None, :])
            q0 = R.quantize_row(Q.GGML_Q8_0, row).reshape(K // 32, 34)
            assert np.array_equal(q0[:, 0:2].copy().view(np.float16)[:, 0].astype(np.float32).view(np.uint32), mine["d0"][0].view(np.uint32)), (name, r)
            assert np.array_equal(q0[:, 2:].copy().view(np.int8).reshape(-1), mine["q80"][0]), (name, r)
            q1 = R.quantize_row(Q.GGML_Q8_1, row).reshape(K // 32, 40)
            assert np.array_equal(q1[:, 0:4].copy().view(np.uint32)[:, 0], mine["d1"][0].view(np.uint32)), (name, r)
            assert np.array_equal(q1[:, 4:8].copy().view(np.uint32)[:, 0], mine["s1"][0].view(np.uint32)), (name, r)
            assert np.array_equal(q1[:, 8:].copy().view(np.int8).reshape(-1), mine["q80"][0]), (name, r)
            assert np.array_equal(mine["sum0"][0], mine["q80"][0].astype(np.int64).reshape(-1, 32).sum(axis=1))
            assert np.array_equal(R.quantize_row(Q.GGML_F16, row).view(np.uint16), A.planes(row[None, :], A.ACT_F16)["xh"][0]), (name, r)


def test_q16_holds_the_q8k_values_in_the_documented_fragment_order():
    v = A.rows(1024, 3)[0]
    p = A.q8k_planes(v)
    q, h = p["q8k"].reshape(3, 4, 256), p["q16"].view(np.float16).reshape(3, 4, 32, 8)
    for c in range(32):
        pp, uu, d = c >> 3, (c >> 2) & 1, c & 3
        e0 = 64 * pp + 16 * uu + 4 * d
        for j, off in enumerate((0, 2, 1, 3, 32, 34, 33, 35)):
            assert np.array_equal(h[:, :, c, j].astype(np.int64), q[:, :, e0 + off])
    assert sorted(A.Q16_ORDER.tolist()) == list(range(256))


def test_no_row_is_ambiguous_for_the_rms_mean():
    for K, N in SHAPES:
        for r, row in enumerate(A.rows(K, N)[0]):
            assert not A.rms_mean(row)[1], (K, N, r)
    for N, K in A.SLAB_SHAPES:
        for ks in A.KS:
            for with_res in (False, True):
                s, res = A.slab_case(ks, N * K, A.slab_stride(N * K))
                x = A.slab_sum32(s[:, :N * K], res if with_res else None).reshape(N, K)
                assert np.isfinite(x).all()
                for r in range(N):
                    assert not A.rms_mean(x[r])[1], (N, K, ks, with_res, r)


def test_every_family_sits_in_a_first_a_last_and_a_second_pass_block():
    first, last, second, q8k_first, q8k_last = set(), set(), set(), set(), set()
    for K, N in SHAPES:
        for lay in A.rows(K, N)[1]:
            if isinstance(lay, int):
                continue
            first.add(lay[0]), last.add(lay[-1]), second.update(lay[16:])
            if K % 256 == 0:
                q8k_first.add(lay[0]), q8k_last.add(lay[-1])
    every = set(range(len(A.FAMILIES)))
    assert first == every and last == every and second == every and q8k_first == every and q8k_last == every
    for N in (3, 5):                                             # the row-level families
        x, lay = A.rows(5120, N)
        assert A.ROW_ZERO in lay and not x[lay.index(A.ROW_ZERO)].any()
    x, lay = A.rows(5120, 5)
    r = x[lay.index(A.ROW_LAST)]
    assert r[-1] != 0 and not r[:-1].any()
    lay = A.rows(13824, 1)[1][0]                                 # magnitudes 1e-30 and 3e4 in neighbouring blocks
    assert A.FAMILIES.index("big") - A.FAMILIES.index("tiny") == 1 and any(lay[i] == A.FAMILIES.index("tiny") and lay[i + 1] == A.FAMILIES.index("big") for i in range(len(lay) - 1))


def test_families_are_what_their_names_say():
    rng = np.random.default_rng(5)
    for name, sums in (("int_a", A.SUMS_A), ("int_b", A.SUMS_B)):
        b = A._block(name, rng)
        p = A.q8k_planes(b[None, :])
        assert p["dk"][0, 0] == 1.0 and np.array_equal(p["q8k"][0].astype(np.float32), b)                  # iscale 1: the values are the integers
        assert tuple(b.reshape(8, 32).sum(axis=1).astype(int)) == sums
    assert sorted(set(A.SUMS_A + A.SUMS_B)) == [-4096, -129, -128, -127, -1, 0, 1, 127, 128, 4064]
    b = A._block("half_k", rng)
    p = A.q8k_planes(b[None, :])
    assert p["dk"][0, 0] == 1.0 and ((b - np.floor(b)) == 0.5).sum() == 255 and (p["q8k"][0][b == 127.5] == 127).all() and (p["q8k"][0][b == -127.5] == -128).all()
    b = A._block("half_80", rng)
    p = A.q80_planes(b[None, :])
    assert (p["d1"] == 1.0).all() and ((b - np.floor(b)) == 0.5).sum() == 248
    for name in ("tie_pn", "tie_np", "tie_thread_pn", "tie_thread_np", "tie_lane0_63_pn", "tie_lane0_63_np", "tie_last_elem"):
        b = A._block(name, rng)
        at = np.nonzero(np.abs(b) == np.abs(b).max())[0]
        assert at.size == 2 and b[at[0]] == -b[at[1]], name
        q = A.q8k_planes(b[None, :])["q8k"][0]
        assert q[at[0]] == -128 and q[at[1]] == 127, name                                                  # the first wins, the second is clamped
        assert (at[0] // 4 == at[1] // 4) == ("thread" in name)
    b = A._block("tie_lane0_63_pn", rng)
    assert abs(b[2]) == np.abs(b).max() == abs(b[253])
    b = A._block("tie_last_elem", rng)
    assert np.nonzero(np.abs(b) == np.abs(b).max())[0].tolist() == [100, 255]
    b = A._block("negmax", rng)
    assert b[np.abs(b).argmax()] < 0
    t, g = A._block("tiny", rng), A._block("big", rng)
    assert np.abs(t).max() / 127 > 2.0 ** -126 and np.abs(t).max() < 2e-30 and np.abs(g).max() == 3e4
    assert np.isfinite(A.q80_planes(g[None, :])["d0"]).all() and (A.q80_planes(t[None, :])["d1"] > 2.0 ** -126).all()
    assert np.signbit(A._block("negzero", rng)).all()
    a, _ = A.silu_operands(13824, 5)                             # every finite fp16 pattern, and the rounding boundaries
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
    exact = h.astype(np.float32) == a
    assert set(A.FINITE_BITS.tolist()) <= set(h[exact].view(np.uint16).tolist()) and np.isfinite(h).all()
    off = a[~exact].astype(np.float64)
    with np.errstate(over="ignore"):
        lo_, hi_ = np.nextafter(h[~exact], np.float16(-np.inf)).astype(np.float64), np.nextafter(h[~exact], np.float16(np.inf)).astype(np.float64)
    hf = h[~exact].astype(np.float64)
    ties = (off - hf == (hi_ - hf) / 2) | (off - hf == (lo_ - hf) / 2)
    assert ties.sum() > 1000 and (~ties).sum() > 1000


def _wrong_planes(v, mask, wrong):
    good, bad = A.planes(v, mask), A.planes(v, mask, wrong=wrong)
    return {k for k in good if not np.array_equal(good[k], bad[k])}


@pytest.mark.parametrize("wrong", [w for w in A.WRONG_RULES if A.WRONG_RULES[w] != ("sum",)])
def test_every_wrong_quantiser_rule_shows_in_the_plane_it_governs(wrong):
    """on the plain rows: the prepared values there are the families themselves"""
    changed = set()
    for K, N in ((256, 1), (1024, 3), (4352, 5), (5120, 5), (352, 5), (32, 5)):
        changed |= _wrong_planes(A.rows(K, N)[0], 15 if K % 256 == 0 else 14, wrong)
    assert set(A.WRONG_RULES[wrong]) <= changed, (wrong, changed)


@pytest.mark.parametrize("wrong", ["slab_reverse", "residual_first"])
def test_every_wrong_summation_order_changes_the_slab_sums(wrong):
    for ks in A.KS:
        if wrong == "slab_reverse" and ks == 2:
            continue                                             # two terms commute
        n = 5120
        s, res = A.slab_case(ks, n, A.slab_stride(n))
        good, bad = A.slab_sum32(s[:, :n], res), A.slab_sum32(s[:, :n], res, wrong=wrong)
        assert (good != bad).sum() > n // 100, (wrong, ks)
        assert A.bound_ratio(good, s[:, :n], res) <= 1.0 and A.bound_ratio(bad, s[:, :n], res) <= 1.0       # both orders are fp32 sums: the bound holds, only the bits tell
        assert np.isnan(s[:, n:]).all() and s[:, n:].size


def test_bound_ratio_is_as_documented():
    s = np.array([[1.0, 0.0], [2.0, 0.0]], np.float32)
    assert A.bound_ratio(np.array([3.0, 0.0]), s) == 0.0
    assert A.bound_ratio(np.array([3.0 + 9 * A.U, 0.0]), s) == pytest.approx(1.0)                           # (2 + 1) * 2^-24 * 3
    assert A.bound_ratio(np.array([3.0, 1e-30]), s) == float("inf") and A.bound_ratio(np.array([np.nan, 0.0]), s) == float("inf")


# ---------------------------------------------------------------------------------------------------------------- the hooks' refusals
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_prepare_hooks_refuse_bad_arguments_before_touching_a_device(lib):
    L = lib.library
    x = np.zeros((2, 512), np.float32)
    none13 = [None] * 13
    f = L.minigpt4_amd_test_prepare
    fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))   # noqa: E731
    bad = [(0, None, 2, 512, 1, 0), (2, x, 2, 512, 1, 0), (-1, x, 2, 512, 1, 0), (0, x, 0, 512, 1, 0), (0, x, 2, 510, 8, 0), (0, x, 2, 0, 8, 0), (0, x, 2, 384, 1, 0),
           (0, x, 2, 384, 3, 0), (0, x, 2, 48, 2, 0), (1, x, 2, 48, 2, 0), (0, x, 2, 512, 0, 0), (0, x, 2, 512, 16, 0), (0, x, 2, 512, 1, 8), (0, x, 2, 512, 1, 2), (0, x, 2, 512, 1, -1)]
    for launcher, xx, N, K, mask, planes in bad:
        assert f(launcher, fp(xx), None, N, K, mask, planes, 0, None, *none13) == 1, (launcher, N, K, mask, planes)
    g = L.minigpt4_amd_test_prepare_slabs
    s1, s2, w, tab, xo = np.zeros((2, 1024), np.float32), np.zeros((2, 2, 1024), np.float32), np.ones(512, np.float32), np.zeros(65536, np.uint16), np.zeros((3, 512), np.float32)
    res = np.zeros((2, 512), np.float32)
    ok0 = dict(launcher=0, slabs=s1, ks=2, stride=1024, residual=None, in_place=0, w=w, N=2, K=512, mask=1, planes=0, tab=None, x_out=xo)
    ok1 = dict(launcher=1, slabs=s2, ks=2, stride=1024, residual=None, in_place=0, w=None, N=2, K=512, mask=1, planes=0, tab=tab, x_out=None)
    changes = [(ok0, dict(slabs=None)), (ok0, dict(launcher=2)), (ok0, dict(ks=1)), (ok0, dict(ks=17)), (ok0, dict(stride=1020)), (ok0, dict(stride=1026, K=513)), (ok0, dict(stride=1022)),
               (ok0, dict(w=None)), (ok0, dict(x_out=None)), (ok0, dict(in_place=1)), (ok0, dict(N=0)), (ok0, dict(K=384)), (ok0, dict(mask=0)), (ok0, dict(planes=2)),
               (ok1, dict(tab=None)), (ok1, dict(residual=res)), (ok1, dict(w=w)), (ok1, dict(x_out=xo)), (ok1, dict(in_place=1)), (ok1, dict(mask=2, K=48, stride=96))]
    for base, ch in changes:
        a = dict(base, **ch)
        rc = g(a["launcher"], fp(a["slabs"]), a["ks"], a["stride"], fp(a["residual"]), a["in_place"], fp(a["w"]), a["N"], a["K"], a["mask"], a["planes"], _p(a["tab"]), fp(a["x_out"]),
               *none13)
        assert rc == 1, ch
    for name, (shape, dtype) in lib.act_plane_shapes(2, 512).items():                                       # the wrapper's planes are what the header says
        assert shape[0] == 3 and np.dtype(dtype).itemsize * int(np.prod(shape[1:])) == {"q8k": 512, "dk": 8, "bsk": 64, "bsq": 32, "bs16": 64, "q16": 1024, "q80": 512, "d0": 64,
                                                                                         "d1": 64, "s1": 64, "sum0": 64, "xh": 1024, "xf": 2048}[name]
    assert tuple(lib.act_plane_shapes(1, 32)) == A.PLANES == lib.ACT_PLANES


def test_slab_hooks_refuse_bad_arguments_before_touching_a_device(lib):
    L = lib.library
    fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))   # noqa: E731
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))   # noqa: E731
    f = L.minigpt4_amd_test_slab_flush
    slabs, res, y = np.zeros((9, 64), np.float32), np.zeros((3, 64), np.float32), np.zeros((4, 64), np.float32)
    ok = dict(n=3, mixed=0, mks=[2, 2, 2], slabs=slabs, stride=64, res=res, rmask=5, y=y)
    changes = [dict(mks=None), dict(slabs=None), dict(y=None), dict(n=0), dict(n=4), dict(stride=0), dict(stride=62), dict(rmask=8), dict(rmask=-1), dict(res=None), dict(mks=[2, 2, 3]),
               dict(mks=[2, 2, 1]), dict(mks=[1, 1, 1]), dict(mks=[2, 17, 2]), dict(mixed=1, mks=[1, 2, 2]), dict(mixed=1, mks=[2, 0, 2]), dict(mixed=1, mks=[2, 2, 17])]
    for ch in changes:
        a = dict(ok, **ch)
        assert f(a["n"], a["mixed"], ip(a["mks"]), fp(a["slabs"]), a["stride"], fp(a["res"]), a["rmask"], fp(a["y"])) == 1, ch
    g = L.minigpt4_amd_test_rope_kv_slabs
    q, kc, vc, v = np.zeros((3, 128), np.float32), np.zeros((16, 128), np.uint16), np.zeros((16, 128), np.uint16), np.zeros((2, 128), np.float32)
    sl = np.zeros((6, 256), np.float32)
    ok = dict(n_head=2, hd=64, n_ctx=16, N=2, pos0=14, mks=[2, 2, 2], slabs=sl, stride=256, v=None, q=q, kc=kc, vc=vc)
    changes = [dict(mks=None), dict(slabs=None), dict(q=None), dict(kc=None), dict(vc=None), dict(n_head=0), dict(hd=0), dict(hd=63), dict(N=0), dict(pos0=-1), dict(pos0=15),
               dict(n_ctx=0), dict(stride=252), dict(stride=258), dict(mks=[1, 2, 2]), dict(mks=[2, 1, 2]), dict(mks=[2, 2, 0]), dict(mks=[2, 2, 17]), dict(mks=[2, 2, 1]), dict(v=v)]
    for ch in changes:
        a = dict(ok, **ch)
        rc = g(a["n_head"], a["hd"], a["n_ctx"], a["N"], a["pos0"], ip(a["mks"]), fp(a["slabs"]), a["stride"], fp(a["v"]), fp(a["q"]), _p(a["kc"]), _p(a["vc"]))
        assert rc == 1, ch
