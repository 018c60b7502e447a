"""The activation-preparation kernels (k_rms_quant, k_silu_mul_quant) and the consumers of a deferred split-K combine (k_rms_quant_slabs, k_silu_mul_quant_slabs,
launch_slab_flush in both forms, launch_slab_reduce, k_rope_kv_slabs with a slab count per matrix), each alone, one launch per hook call, against tests/act_ref.py.

No tolerance is measured here: a plane either equals the reference BIT FOR BIT -- tests/test_cpu_act_ref.py shows that the reference agrees with the oracle's quantize_row,
that no row of these inputs is ambiguous for the rms mean, and that the inputs tell each wrong rule from the right one -- or, for the slab sums, lies within the derived bound
(ks + 1) * 2^-24 * sum |terms| of the float64 sum as well.  Every hook call also checks the guard row of every plane and that the planes `mask` does not select keep their fill."""
import numpy as np
import pytest

import act_ref as A

pytestmark = pytest.mark.gpu
FILL = 0xFF
ALL_OPT = A.PLANE_BSQ | A.PLANE_BS16 | A.PLANE_Q16
RMS, SILU = 0, 1


def _table():
    import refcpu as R
    return R.table(1)


@pytest.fixture(scope="module")
def computed_silu(gpu_lib):
    """the computed SiLU arm on all 65 536 fp16 bit patterns, as this device evaluates it (held to float64 by tests/test_gpu_activations.py)"""
    return gpu_lib.amd_test_activation(1, None)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _where(name, got, want, layout):
    """a readable first difference: plane, row, element, and the family of the block it lies in (rows built from act_ref.FAMILIES only)"""
    g, w = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    r, i = [int(v[0]) for v in np.nonzero(g != w)]
    fam = "-"
    if layout is not None and not isinstance(layout[r], int):
        fam = A.FAMILIES[layout[r][i * len(layout[r]) // g.shape[1]]]
    return "%s row %d element %d (%s): got %r, want %r; %d of %d differ" % (name, r, i, fam, g[r, i], w[r, i], int((g != w).sum()), g.size)


def _check(outs, want, N, layout=None, what=""):
    """selected planes == the reference bit for bit; guard rows and every other plane at the fill"""
    for name in A.PLANES:
        got = outs[name]
        if name in want:
            w = np.ascontiguousarray(want[name])
            assert got.dtype == w.dtype and got[:N].shape == w.shape, (what, name, got.dtype, w.dtype, got.shape, w.shape)
            if not np.array_equal(_bytes(got[:N]), _bytes(w)):
                bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
                raise AssertionError("%s: %s" % (what, _where(name, got[:N].view(bits), w.view(bits), layout)))
            assert (_bytes(got[N:]) == FILL).all(), (what, name, "guard row")
        else:
            assert (_bytes(got) == FILL).all(), (what, name, "a plane the mask does not select was written")


def _masks(K):
    return [m for m in A.MASKS if not (m & A.ACT_Q8K and K % 256)]


def _combos(K):
    """(mask, optional planes): every optional set with every mask that holds ACT_Q8K (no other mask writes them)"""
    return [(m, o) for m in _masks(K) for o in (A.OPTIONALS if m & A.ACT_Q8K else (0,))]


def _forms(K, N, computed_silu):
    """name -> (launcher, x, second, table, prepared values) of the five forms of the two launchers"""
    x, layout = A.rows(K, N)
    a, b = A.silu_operands(K, N)
    w = A.norm_weight(K)
    return {"rms_plain": (RMS, x, None, None, x, layout), "rms_norm": (RMS, x, w, None, A.rms_values(x, w), layout), "silu_plain": (SILU, x, None, None, x, layout),
            "silu_table": (SILU, a, b, _table(), A.silu_values(a, b, _table()), None), "silu_computed": (SILU, a, b, None, A.silu_values(a, b, computed_silu), None)}


@pytest.mark.parametrize("K", A.K_32)
def test_prepare_every_plane_equals_the_reference(gpu_lib, computed_silu, K):
    for N in A.NS:
        for form, (launcher, x, second, table, values, layout) in _forms(K, N, computed_silu).items():
            full = A.planes(values, 15 if K % 256 == 0 else 14)
            for mask, opt in _combos(K):
                want = A.planes(values, mask, opt)
                assert all(np.array_equal(_bytes(want[k]), _bytes(full[k])) for k in want)               # (one reference, the mask only selects)
                rc, outs = gpu_lib.amd_test_prepare(launcher, x, second, mask=mask, planes=opt, silu_table=table)
                assert rc == 0, (form, K, N, mask, opt, rc)
                _check(outs, want, N, layout, "%s K=%d N=%d mask=%d planes=%d" % (form, K, N, mask, opt))


@pytest.mark.parametrize("K", A.K_32)
def test_prepare_sequential_sum_gives_the_same_bits(gpu_lib, K):
    """no row of these inputs is ambiguous (tests/test_cpu_act_ref.py): the one-thread sum and the parallel one must land on the same mean"""
    mask = 15 if K % 256 == 0 else 14
    for N in A.NS:
        x, layout = A.rows(K, N)
        w = A.norm_weight(K)
        want = A.planes(A.rms_values(x, w), mask)
        for seq in (False, True):
            rc, outs = gpu_lib.amd_test_prepare(RMS, x, w, mask=mask, planes=ALL_OPT, sequential_sum=seq)
            assert rc == 0
            _check(outs, want, N, layout, "rms_norm sequential=%d K=%d N=%d" % (seq, K, N))


@pytest.mark.parametrize("K", A.K_32)
def test_prepare_rows_do_not_depend_on_their_neighbours(gpu_lib, K):
    """five rows in one launch == five one-row launches (no cross-row state)"""
    mask = 15 if K % 256 == 0 else 14
    x, _ = A.rows(K, 5)
    a, b = A.silu_operands(K, 5)
    w = A.norm_weight(K)
    for launcher, xx, second, table in ((RMS, x, w, None), (RMS, x, None, None), (SILU, a, b, _table()), (SILU, a, b, None)):
        rc, outs = gpu_lib.amd_test_prepare(launcher, xx, second, mask=mask, planes=ALL_OPT, silu_table=table)
        assert rc == 0
        for r in range(5):
            rc, one = gpu_lib.amd_test_prepare(launcher, xx[r:r + 1], second if launcher == RMS or second is None else second[r:r + 1], mask=mask, planes=ALL_OPT, silu_table=table)
            assert rc == 0
            for name in A.PLANES:
                assert np.array_equal(_bytes(one[name][0]), _bytes(outs[name][r])), (launcher, K, r, name)


# ---------------------------------------------------------------------------------------------------------------- the consumers of a deferred combine
_RATIOS = {}


def _note_ratio(case, got, slabs, residual=None):
    r = A.bound_ratio(got, slabs, residual)
    _RATIOS[case] = max(r, _RATIOS.get(case, 0.0))
    print("slab sum error / bound, %s: %.4f" % (case, r))
    assert r <= 1.0, (case, r)


@pytest.mark.parametrize("shape", A.SLAB_SHAPES, ids=lambda s: "N%d_K%d" % s)
@pytest.mark.parametrize("ks", A.KS)
def test_rms_quant_slabs(gpu_lib, shape, ks):
    N, K = shape
    n = N * K
    slabs, res = A.slab_case(ks, n, A.slab_stride(n))
    w = A.norm_weight(K)
    runs = {}
    for how, residual, in_place in (("none", None, False), ("separate", res, False), ("in_place", res, True)):
        x_ref = A.slab_sum32(slabs[:, :n], residual).reshape(N, K)
        want = A.planes(A.rms_values(x_ref, w), 15)
        rc, x_out, outs = gpu_lib.amd_test_prepare_slabs(RMS, slabs, N, K, residual=residual, in_place=in_place, w=w, mask=15, planes=ALL_OPT)
        assert rc == 0, (how, rc)
        what = "rms slabs %s N=%d K=%d ks=%d" % (how, N, K, ks)
        assert np.array_equal(_bytes(x_out[:N]), _bytes(x_ref)), what + ": x_out is not the fp32-ordered sum"       # (NaN padding: a NaN anywhere would fail here)
        assert (_bytes(x_out[N:]) == FILL).all(), what + ": x_out guard row"
        _note_ratio("rms_quant_slabs ks=%d %s" % (ks, how), x_out[:N], slabs[:, :n], residual)
        _check(outs, want, N, None, what)
        rc, again = gpu_lib.amd_test_prepare(RMS, x_out[:N], w, mask=15, planes=ALL_OPT)                            # the planes of k_rms_quant on that x_out
        assert rc == 0
        for name in A.PLANES:
            assert np.array_equal(_bytes(again[name]), _bytes(outs[name])), (what, name)
        runs[how] = (x_out, outs)
        for mask, opt in ((A.ACT_Q8K, 0), (A.ACT_Q80, 0), (A.ACT_F16 | A.ACT_F32, 0)):                               # the mask selects here as it does in k_rms_quant
            rc, x2, o2 = gpu_lib.amd_test_prepare_slabs(RMS, slabs, N, K, residual=residual, in_place=in_place, w=w, mask=mask, planes=opt)
            assert rc == 0 and np.array_equal(_bytes(x2), _bytes(x_out))
            _check(o2, A.planes(A.rms_values(x_ref, w), mask, opt), N, None, what + " mask=%d" % mask)
    for name in A.PLANES:
        assert np.array_equal(_bytes(runs["separate"][1][name]), _bytes(runs["in_place"][1][name])), name
    assert np.array_equal(_bytes(runs["separate"][0]), _bytes(runs["in_place"][0]))


@pytest.mark.parametrize("shape", A.SLAB_SHAPES, ids=lambda s: "N%d_K%d" % s)
@pytest.mark.parametrize("ks", A.KS)
def test_silu_mul_quant_slabs(gpu_lib, shape, ks):
    N, K = shape
    n = N * K
    stride = A.slab_stride(n)
    slabs = np.stack([A.slab_case(ks, n, stride, tag)[0] for tag in (1, 2)])
    a, b = (A.slab_sum32(slabs[m][:, :n]).reshape(N, K) for m in (0, 1))
    table = _table()
    values = A.silu_values(a, b, table)
    assert np.isfinite(values).all()
    for mask, opt in ((15, ALL_OPT), (A.ACT_Q8K, A.PLANE_BSQ), (A.ACT_Q80, 0)):
        what = "silu slabs N=%d K=%d ks=%d mask=%d" % (N, K, ks, mask)
        rc, x_out, outs = gpu_lib.amd_test_prepare_slabs(SILU, slabs, N, K, mask=mask, planes=opt, silu_table=table)
        assert rc == 0 and x_out is None, what
        _check(outs, A.planes(values, mask, opt), N, None, what)
        rc, again = gpu_lib.amd_test_prepare(SILU, a, b, mask=mask, planes=opt, silu_table=table)                    # k_silu_mul_quant on those sums
        assert rc == 0
        for name in A.PLANES:
            assert np.array_equal(_bytes(again[name]), _bytes(outs[name])), (what, name)
    for m in (0, 1):
        _note_ratio("silu_mul_quant_slabs ks=%d operand %d" % (ks, m), (a, b)[m], slabs[m][:, :n])                   # (what the reference sums; the planes above prove the kernel formed the same)


FLUSH_STRIDES = (4, 1028, 3 * 4352)                              # one thread; one workgroup and a thread; 12.75 workgroups


@pytest.mark.parametrize("stride", FLUSH_STRIDES)
@pytest.mark.parametrize("ks", A.KS)
def test_slab_flush_plain(gpu_lib, stride, ks):
    for n in (1, 2, 3):
        cases = [A.slab_case(ks, stride, stride, 10 + i) for i in range(n)]
        slabs = np.concatenate([c[0] for c in cases])
        res = np.stack([c[1] for c in cases])
        for rmask in sorted({0, 1, (1 << n) - 1, 1 << (n - 1)}):
            rc, y = gpu_lib.amd_test_slab_flush([ks] * n, slabs, stride, residual=res if rmask else None, residual_mask=rmask)
            assert rc == 0, (n, rmask, rc)
            for i in range(n):
                r = res[i] if rmask >> i & 1 else None
                assert np.array_equal(_bytes(y[i]), _bytes(A.slab_sum32(cases[i][0], r))), ("plain flush", stride, ks, n, rmask, i)
                _note_ratio("slab_flush plain ks=%d" % ks, y[i], cases[i][0], r)
            assert (_bytes(y[n]) == FILL).all()


@pytest.mark.parametrize("stride", FLUSH_STRIDES)
@pytest.mark.parametrize("mks", A.MIXED_KS, ids=lambda m: "mks%d%d%d" % m)
def test_slab_flush_mixed(gpu_lib, stride, mks):
    """q | k pending with one count, v pending with another or already in place (then it must come back bit for bit, residual or not)"""
    cases = [A.slab_case(max(2, k), stride, stride, 20 + i) for i, k in enumerate(mks)]
    slabs = np.concatenate([c[0] for c, k in zip(cases, mks) if k > 1])
    res = np.stack([c[1] for c in cases])
    v_here = (np.random.default_rng(7).standard_normal(stride) * 0.7).astype(np.float32)
    v_here[::7] = -0.0
    for rmask in (0, 7, 4):
        rc, y = gpu_lib.amd_test_slab_flush(mks, slabs, stride, mixed=True, residual=res if rmask else None, residual_mask=rmask, in_place={2: v_here} if mks[2] == 1 else None)
        assert rc == 0, (mks, rmask, rc)
        for i, k in enumerate(mks):
            if k == 1:
                assert np.array_equal(_bytes(y[i]), _bytes(v_here)), ("mixed flush touched the matrix that is in place", stride, mks, rmask)
                continue
            r = res[i] if rmask >> i & 1 else None
            assert np.array_equal(_bytes(y[i]), _bytes(A.slab_sum32(cases[i][0], r))), ("mixed flush", stride, mks, rmask, i)
            _note_ratio("slab_flush mixed ks=%d" % k, y[i], cases[i][0], r)
        assert (_bytes(y[3]) == FILL).all()


@pytest.mark.parametrize("ks", A.KS)
def test_a_deferred_combine_and_a_flushed_one_yield_identical_rows(gpu_lib, ks):
    """MINIGPT4_DEFER_COMBINE's promise: x = residual + slabs formed by k_rms_quant_slabs == the same slabs flushed by launch_slab_flush, then k_rms_quant on it"""
    N, K = A.SLAB_SHAPES[1]
    n = N * K
    slabs, res = A.slab_case(ks, n, A.slab_stride(n))
    w = A.norm_weight(K)
    rc, x_out, outs = gpu_lib.amd_test_prepare_slabs(RMS, slabs, N, K, residual=res, w=w, mask=15, planes=ALL_OPT)
    assert rc == 0
    rc, y = gpu_lib.amd_test_slab_flush([ks], np.ascontiguousarray(slabs[:, :n]), n, residual=res[None, :], residual_mask=1)
    assert rc == 0 and np.array_equal(_bytes(y[0]), _bytes(x_out[:N]))
    rc, flushed = gpu_lib.amd_test_prepare(RMS, y[0].reshape(N, K), w, mask=15, planes=ALL_OPT)
    assert rc == 0
    for name in A.PLANES:
        assert np.array_equal(_bytes(flushed[name]), _bytes(outs[name])), name


@pytest.mark.parametrize("hd", (64, 128))
@pytest.mark.parametrize("mks", A.MIXED_KS, ids=lambda m: "mks%d%d%d" % m)
def test_rope_kv_slabs_with_a_count_per_matrix(gpu_lib, hd, mks):
    """the rotated q and both caches == the plain k_rope_kv (one side of minigpt4_amd_test_rope_kv_seg, held to float64 by tests/test_gpu_attn_kernels.py) fed the
    fp32-ordered sums; positions 0, 1 and n_ctx - 1 among the rows"""
    n_head, n_ctx = 2, 16
    E = n_head * hd
    for pos0, N in ((0, 3), (n_ctx - 1, 1), (n_ctx - 3, 3)):
        n = N * E
        stride = A.slab_stride(n)
        cases = [A.slab_case(max(2, k), n, stride, 30 + i) for i, k in enumerate(mks)]
        sums = [A.slab_sum32(c[0][:, :n]).reshape(N, E) for c in cases]
        v_here = None
        if mks[2] == 1:
            v_here = sums[2] = (np.random.default_rng(8).standard_normal((N, E)) * 0.7).astype(np.float32)
        slabs = np.concatenate([c[0] for c, k in zip(cases, mks) if k > 1])
        rc, q, kc, vc = gpu_lib.amd_test_rope_kv_slabs(n_head, hd, n_ctx, N, pos0, mks, slabs, stride, v_in_place=v_here)
        assert rc == 0, (hd, mks, pos0, rc)
        _, (q_ref, kc_ref, vc_ref) = gpu_lib.amd_test_rope_kv_seg(n_head, n_ctx, 1, [(0, N, pos0)], sums[0], sums[1], sums[2], ks=1)
        what = ("rope_kv_slabs", hd, mks, pos0, N)
        assert np.isfinite(q[:N]).all() and np.array_equal(_bytes(q[:N]), _bytes(q_ref)), what
        assert (_bytes(q[N:]) == FILL).all(), what
        assert np.array_equal(_bytes(kc), _bytes(kc_ref[0])) and np.array_equal(_bytes(vc), _bytes(vc_ref[0])), what
        assert kc[pos0:pos0 + N].any() and vc[pos0:pos0 + N].any() and not kc[:pos0].any() and not kc[pos0 + N:].any()
        for i, k in enumerate(mks):
            if k > 1:
                _note_ratio("rope_kv_slabs ks=%d" % k, sums[i], cases[i][0][:, :n])
