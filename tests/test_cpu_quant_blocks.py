"""tests/quant_blocks.py held to the oracle, no GPU: (1) its float64 decoders agree with the oracle's dequantize_row on random block bytes; (2) its activation rows quantise
exactly; (3) on every input that tests/test_gpu_quant_blocks.py gives a kernel, the ORACLE's mul_mat stays inside the bound (the reference alone -- seen at <= 0.25 of the
bound when the bound was set, at <= 0.36 on the inputs of this module; the assertion is <= 1); (4) every mutant decoder leaves the bound on at least one case of its type -- a mutant that no case catches means the
inputs are too weak (strengthen the generators then, never the bound)."""
import numpy as np
import pytest

import quant_blocks as QB
import refcpu as R

GENS = ("random", "extreme")
SETS = QB.weight_sets()


@pytest.mark.parametrize("t", QB.ALL_TYPES, ids=lambda t: QB.NAMES[t])
@pytest.mark.parametrize("gen", GENS)
def test_float64_decoders_agree_with_the_oracles_dequantize_row(t, gen):
    """two-term forms (w = scale part - min part): the oracle rounds once in fp32 -> one fp32 ulp of a; one-term forms decode exactly"""
    n_rows, K = 7, 1280
    raw = QB.blocks(gen, t, n_rows, K)
    w, a = QB.decode(t, raw, n_rows * K)
    assert (a >= np.abs(w)).all() and np.isfinite(w).all()
    ref = R.dequantize_row(t, raw.reshape(-1), n_rows * K).astype(np.float64)
    if t in QB.TWO_TERM:
        assert (np.abs(ref - w) <= np.spacing(a.astype(np.float32)).astype(np.float64)).all()
        assert (ref != w).sum() < 0.9 * w.size                                   # (and not vacuous)
    else:
        assert np.array_equal(ref, w)
    if gen == "random":                                                          # every field value and both signs of w occur
        assert (w > 0).any() and (w < 0).any() and (w == 0).any()


def test_generated_fields_are_finite_and_cover_the_value_set():
    for t in QB.F16_FIELDS:
        b = QB.blocks("random", t, 7, 1280).reshape(-1, QB.BLOCK[t][1])
        for off in QB.F16_FIELDS[t]:
            f = np.ascontiguousarray(b[:, off:off + 2]).view(np.float16)[:, 0]
            assert np.isfinite(f).all() and set(f.view(np.uint16).tolist()) <= set(QB.FIELD_VALUES.view(np.uint16).tolist())
            assert (f > 0).any() and (f < 0).any() and (f == 0).any() and (np.abs(f) == np.float16(2.0 ** -24)).any()
        e = QB.blocks("extreme", t, 70, 1024).reshape(70, -1, QB.BLOCK[t][1])
        d = np.ascontiguousarray(e[:, :, QB.F16_FIELDS[t][0]:QB.F16_FIELDS[t][0] + 2]).view(np.float16)[:, :, 0]
        assert np.isfinite(d).all() and (np.sign(d[0, 1:]) == -np.sign(d[0, :-1])).all()      # d alternates in sign from block to block
        last = e[69]
        assert sum(not np.array_equal(last[i], last[0]) for i in range(last.shape[0])) == 1   # one block differs from its neighbours, and it is not the first


@pytest.mark.parametrize("t,K", [(t, K) for t in (QB.Q4_K, QB.Q4_0, QB.F16, QB.F32) for K in (256, 352, 512, 1024, 1280, 2048, 4096, 5120, 13824) if K % 256 == 0 or t != QB.Q4_K],
                         ids=lambda v: QB.NAMES[v] if v < 256 else str(v))
def test_activation_rows_quantise_exactly(t, K):
    """Q8_K: d = 1 and the int8 values are the row (d = 0 on an all-zero block); Q8_0 / Q8_1: d = 1; fp16 / fp32: the row itself"""
    from minigpt4_cpp_amd import quants as Q
    x = QB.activation_rows(t, K)
    assert x.shape == (QB.N_ACT, K) and np.array_equal(x, np.rint(x))
    kq = t in QB.K_TYPES
    assert x.min() == (-128 if kq else -127) and x.max() == 127
    if kq:
        assert (x[0] == -128).all() and (x[1].reshape(-1, 256).min(axis=1) == -128).all() and (x[4].reshape(-1, 256)[K // 512] == 0).all() and not x[5, 256:].any()
    for row in x:
        if kq:
            q = R.quantize_row(Q.GGML_Q8_K, row).reshape(K // 256, 292)
            d, qs, bs = q[:, 0:4].copy().view(np.float32)[:, 0], q[:, 4:260].copy().view(np.int8), q[:, 260:292].copy().view(np.int16)
            blocks = row.reshape(-1, 256)
            assert np.array_equal(d, np.where(np.abs(blocks).max(axis=1) > 0, 1.0, 0.0)) and np.array_equal(qs, blocks)
            assert np.array_equal(bs, blocks.reshape(-1, 16, 16).sum(axis=2))
        elif t in (QB.F16, QB.F32):
            qt = Q.GGML_F16 if t == QB.F16 else Q.GGML_F32
            got = R.quantize_row(qt, row).view(np.float16 if t == QB.F16 else np.float32)
            assert np.array_equal(got.astype(np.float32), row)
        else:
            blocks = row.reshape(-1, 32)
            want_d = np.where(np.abs(blocks).max(axis=1) > 0, 1.0, 0.0)
            q0 = R.quantize_row(Q.GGML_Q8_0, row).reshape(K // 32, 34)
            assert np.array_equal(q0[:, 0:2].copy().view(np.float16)[:, 0].astype(np.float64), want_d) and np.array_equal(q0[:, 2:].copy().view(np.int8), blocks)
            q1 = R.quantize_row(Q.GGML_Q8_1, row).reshape(K // 32, 40)
            assert np.array_equal(q1[:, 0:4].copy().view(np.float32)[:, 0], want_d) and np.array_equal(q1[:, 8:].copy().view(np.int8), blocks)
            assert np.array_equal(q1[:, 4:8].copy().view(np.float32)[:, 0], blocks.sum(axis=1))


_ORACLE = {}                                                     # (gen, type) -> the oracle's worst ratio, printed by the last test


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("wset", SETS, ids=lambda s: "%s_R%d_K%d" % (QB.NAMES[s[0]], s[1], s[2]))
def test_oracle_stays_inside_the_bound_on_every_gpu_case(gen, wset):
    """The reference alone: the oracle's mul_mat (fp32 sums in ggml's order) on every activation row against every weight set of the GPU cases: ratio <= 1 (seen: <= 0.25 when the bound was set, <= 0.36 on these inputs)."""
    t, n_rows, K = wset
    exact, mag = QB.reference(gen, t, n_rows, K)
    got = R.mul_mat(t, QB.blocks(gen, t, n_rows, K).reshape(-1), K, n_rows, QB.activation_rows(t, K))
    r = QB.ratio_of(got, exact, mag, QB.n_blocks(t, K))
    _ORACLE[(gen, t)] = max(r, _ORACLE.get((gen, t), 0.0))
    print("oracle ratio %s %s R%d K%d: %.4f" % (gen, QB.NAMES[t], n_rows, K, r))
    assert r <= 1.0, (gen, QB.NAMES[t], n_rows, K, r)
    assert r > 0.0                                                # fp32 sums of these inputs do round: a ratio of exactly 0 would mean the comparison is vacuous


def _cases_of(t):
    return [(g, s) for g in GENS for s in SETS if s[0] == t]


@pytest.mark.parametrize("mutant,t", [(m, t) for m, types in QB.MUTANTS.items() for t in types], ids=lambda v: v if isinstance(v, str) else QB.NAMES[v])
def test_every_mutant_leaves_the_bound_on_some_case_of_its_type(mutant, t):
    worst = 0.0
    for gen, (_, n_rows, K) in _cases_of(t):
        exact, mag = QB.reference(gen, t, n_rows, K)
        worst = max(worst, QB.ratio_of(QB.mutant_product(mutant, gen, t, n_rows, K), exact, mag, QB.n_blocks(t, K)))
        if worst > 1.0:
            break
    assert worst > 1.0, (mutant, QB.NAMES[t], worst)


@pytest.mark.parametrize("gen", GENS)
def test_mutants_show_in_the_gathered_rows_too(gen):
    """the embedding gather's check is elementwise (one fp32 ulp of a): every decoder mutant changes some element of the 7-row tables by more than that"""
    for t, K in QB.GET_ROWS_CASES:
        raw = QB.blocks(gen, t, QB.GET_ROWS_TABLE, K)
        w, a = QB.decode(t, raw, QB.GET_ROWS_TABLE * K)
        for m in QB.mutants_of(t):
            if m == "bsum32_high_digit_clamped":
                continue                                          # a property of the product, not of the decoder
            wm, _ = QB.decode(t, raw, QB.GET_ROWS_TABLE * K, m)
            caught = (np.abs(wm - w) > np.spacing(a.astype(np.float32))).any()
            assert caught or gen == "extreme", (m, QB.NAMES[t], K)    # constant patterns may hide a swap; random bytes must not


def test_ratio_treats_a_zero_bound_and_a_residual_as_documented():
    x = np.array([[0.0, 0.0], [1.0, -2.0]])
    w, a = np.array([[0.5, 0.25]]), np.array([[0.5, 0.25]])
    assert QB.ratio(np.array([[0.0], [0.0]]), x, w, a, 1) == 0.0
    assert QB.ratio(np.array([[1e-30], [0.0]]), x, w, a, 1) == float("inf")                 # bound zero: exactly zero or nothing
    assert QB.ratio(np.array([[0.0], [5 * QB.U]]), x, w, a, 1) == pytest.approx(1.0)        # |x| . a = 1, (1 + 4) * 2^-24
    res = np.array([[3.0], [2.0]])
    assert QB.ratio(np.array([[3.0], [2.0]]), x, w, a, 1, residual=res) < 1.0
    assert QB.ratio(np.array([[3.0 + 1e-6], [2.0]]), x, w, a, 1, residual=res) == float("inf")
    assert QB.ratio(np.array([[np.nan], [0.0]]), x, w, a, 1) == float("inf")


def test_get_rows_hook_refuses_bad_arguments_before_touching_a_device(lib):
    """1 for a NULL pointer, a token outside [-1, n_rows), a K that is not a whole number of blocks, an unknown type -- with or without a device"""
    import ctypes
    raw = QB.blocks("random", QB.Q4_K, 7, 256)
    for args in [(QB.Q4_K, raw, 7, 256, [7]), (QB.Q4_K, raw, 7, 256, [0, -2]), (QB.Q4_K, raw, 7, 255, [0]), (QB.Q4_0, raw, 7, 48, [0]), (QB.Q3_K, raw, 7, 128, [0]), (5, raw, 7, 256, [0])]:
        with pytest.raises(ValueError):
            lib.amd_test_get_rows(*args)
    f = lib.library.minigpt4_amd_test_get_rows
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    tok, out = np.zeros(1, np.int32), np.zeros((2, 256), np.float32)
    r8 = np.ascontiguousarray(raw)
    assert f(QB.Q4_K, None, 7, 256, tok.ctypes.data, 1, out.ctypes.data) == 1
    assert f(QB.Q4_K, r8.ctypes.data, 7, 256, None, 1, out.ctypes.data) == 1
    assert f(QB.Q4_K, r8.ctypes.data, 7, 256, tok.ctypes.data, 1, None) == 1
