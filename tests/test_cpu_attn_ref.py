"""tests/attn_ref.py checked without a GPU, on exactly the cases tests/test_gpu_attn_kernels.py runs the kernels on (the case lists live in attn_ref).

  inside the bound   the contract evaluated with fp32 arithmetic where the kernels have it -- three accumulation orders for the scores and for P.V -- stays inside
                     attn_bound against attn_ref in every case, and an fp32 rotation stays inside rope_bound against rope_ref: the bounds ask nothing of a kernel that
                     fp32 arithmetic in some order cannot give;
  not vacuous        every wrong reference of attn_ref.MUTANTS is at least 8 bounds away somewhere, in every case it applies to (a condition on the INPUTS: the needles);
  tables             the restated RoPE iteration is within rope_dtheta of the exact angles at every position up to 2176;
  the model's        with its fp16 rounding points switched off attn_ref is the attention block of tests/f64ref.py.
Each of the first three prints its figure (pytest -s shows them; the assertion messages carry them too)."""
import os

import numpy as np
import pytest

import attn_ref as A
import f64ref

MIN_FACTOR = 8.0
FAMILIES = {
    "decode": (A.DECODE_CASES, A.decode_case, A.body_P),
    "verify": (A.VERIFY_CASES, A.verify_case, A.body_P),
    "split": (A.SPLIT_CASES + [A.SPLIT_WIDE], A.split_case, A.split_P),
    "plain": (A.PLAIN_CASES, A.plain_case, A.body_P),
    "prompt": (A.PROMPT_CASES, A.prompt_case_of, lambda hd: 64),
}


def _hd(case_key):
    return next(x for x in case_key if x in A.HDS)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fp32_emulations_stay_inside_the_bound_in_every_case(family):
    keys, maker, P_of = FAMILIES[family]
    worst = (0.0, None)
    for key in keys:
        case, ref = maker(*key), A.expected_of(maker, *key)
        for order in A.ORDERS:
            got = A.expected(case, emulate=order, P=P_of(_hd(key)))["out"]
            r = A.ratio(got, ref["out"], ref["bound"])
            worst = max(worst, (r, (key, order)), key=lambda x: x[0])
            assert r <= 1.0, (family, key, order, r)
    print(f"\n{family}: largest |fp32 emulation - attn_ref| / attn_bound over {len(keys)} cases x {len(A.ORDERS)} orders = {worst[0]:.3f} at {worst[1]}")
    assert 0.0 < worst[0] <= 1.0, worst


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_mutant_is_at_least_eight_bounds_away_in_every_case_it_applies_to(family):
    keys, maker, _ = FAMILIES[family]
    smallest, seen = (np.inf, None), set()
    for key in keys:
        case, ref = maker(*key), A.expected_of(maker, *key)
        # key-split: steps on one conversation, the last step sees every key the earlier ones see (and up to 17 000 of them): the mutants are measured on it and
        # on the first step (at the end of the cache the last step has no row behind it that a range one too long could read)
        rows = sorted({0, len(case["pos"]) - 1}) if family == "split" else list(range(len(case["pos"])))
        for mutant in A.mutants_of(case):
            r = A.ratio(A.expected(case, mutant, rows=rows)["out"][rows], ref["out"][rows], ref["bound"][rows])
            smallest = min(smallest, (r, (key, mutant)), key=lambda x: x[0])
            seen.add(mutant[0])
            assert r >= MIN_FACTOR, f"{family} {key}: mutant {mutant} is only {r:.2f} bounds away -- strengthen the case's needles"
    print(f"\n{family}: smallest max_d |mutant - attn_ref| / attn_bound over {len(keys)} cases = {smallest[0]:.1f} at {smallest[1]}; mutants seen: {sorted(seen)}")
    assert smallest[0] >= MIN_FACTOR, smallest
    want = set(A.MUTANTS)
    if family == "prompt":                                            # q arrives rotated and every key comes from the cache: nothing of the pass to get wrong
        want -= {"own_key_left_out", "own_key_unrotated", "q_at_pos_minus_1", "q_at_pos_plus_1", "sin_sign", "half_split_pairs", "max_over_cached_only",
                 "verify_reads_stale_cache_row"}
    if family == "decode":                                            # one row per conversation
        want -= {"causal_one_too_long", "causal_one_too_short", "verify_reads_stale_cache_row"}
    if family != "decode":                                            # the own-key-leads cases are listed with the one-row form
        want -= {"max_over_cached_only"}
    assert seen == want, (family, sorted(want - seen), sorted(seen - want))


def test_own_lead_cases_overflow_the_exponential_when_the_maximum_skips_the_own_key():
    """What makes `max_over_cached_only` visible: the own key's score leads every cached key's by more than 11.09, so fp16(exp(.)) of it is infinite."""
    for key in A.DECODE_CASES:
        if key[0] != "one_own_lead":
            continue
        case = A.decode_case(*key)
        bad = A.expected(case, ("max_over_cached_only", None))["out"]
        assert not np.isfinite(bad).any(), key
        assert np.isfinite(A.expected_of(A.decode_case, *key)["out"]).all()


@pytest.mark.parametrize("hd", A.HDS)
def test_fp32_rotation_stays_inside_rope_bound(hd):
    """rope_f32 (the kernels' statements) against rope_ref / rope_bound on the RoPE cases' rows, with the restated table and with a table whose every entry is one fp32
    ulp off (a cosf / sinf that is not correctly rounded); the fp16 cache rows with the half ulp added.  Figures printed."""
    q, k, v, slot, pos = A.rope_case(hd, A.N_HEAD, A.ROPE_SEGS, 600000 + hd)
    tabs = A.rope_tables_ref(A.ROPE_CTX, hd)
    want = A.rope_ref(k, pos, A.N_HEAD, tabs)
    worst = 0.0
    for t in (tabs, tuple(np.nextafter(x, np.float32(2.0)) for x in tabs), tuple(np.nextafter(x, np.float32(-2.0)) for x in tabs)):
        got = A.rope_f32(k, pos, A.N_HEAD, t)
        r32 = A.ratio(got, want, A.rope_bound(k, pos, hd))
        r16 = A.ratio(A.f16(got), want, A.rope_bound(k, pos, hd, cache=True, tables=tabs))
        worst = max(worst, r32, r16)
        assert r32 <= 1.0 and r16 <= 1.0, (hd, r32, r16)
    print(f"\nhd {hd}: largest |fp32 rotation - rope_ref| / rope_bound = {worst:.3f}")
    # not vacuous: the neighbouring position, the wrong sine and the other pairing leave the bound by far, on the fp32 rows and on the fp16 rows
    for name, bad in (("pos + 1", A.rope_f32(k, np.minimum(pos + 1, A.ROPE_CTX - 1), A.N_HEAD, tabs)), ("sin sign", A.rope_f32(k, pos, A.N_HEAD, tabs, sin_sign=-1.0)),
                      ("half split", A.rope_f32(k, pos, A.N_HEAD, tabs, half_split=True))):
        rows = pos > 0 if name != "pos + 1" else pos < A.ROPE_CTX - 1
        assert A.ratio(bad[rows], want[rows], A.rope_bound(k, pos, hd)[rows]) >= 1000.0, name
        assert A.ratio(A.f16(bad[rows]), want[rows], A.rope_bound(k, pos, hd, cache=True, tables=tabs)[rows]) >= MIN_FACTOR, name
    # the neighbouring position at the HIGHEST pair index alone (the slowest angle) still leaves the fp32 bound
    hi = np.zeros(A.N_HEAD * hd, bool); hi.reshape(A.N_HEAD, hd)[:, -2:] = True
    bad = A.rope_f32(k, np.minimum(pos + 1, A.ROPE_CTX - 1), A.N_HEAD, tabs)
    rows = (pos > 0) & (pos < A.ROPE_CTX - 1)
    assert A.ratio(bad[rows][:, hi], want[rows][:, hi], A.rope_bound(k, pos, hd)[rows][:, hi]) >= MIN_FACTOR


@pytest.mark.parametrize("hd", A.HDS)
def test_restated_rope_table_is_within_dtheta_of_the_exact_angles(hd):
    n = 2177
    th, exact, dth = A.rope_thetas_ref(n, hd).astype(np.float64), A.rope_angles_exact(n, hd), A.rope_dtheta(np.arange(n), hd)
    err = np.abs(th - exact)
    assert (err <= dth).all(), float((err / np.maximum(dth, 1e-300)).max())
    used = float((err[1:] / dth[1:]).max())
    print(f"\nhd {hd}: largest |fp32 theta - exact| / dtheta over positions 0 .. {n - 1} = {used:.3f}")
    assert used > 0.01                                                 # ... and dtheta is not orders of magnitude too wide
    c, s = A.rope_tables_ref(n, hd)
    assert (np.abs(c - np.cos(exact)) <= dth + 2.0 ** -24).all() and (np.abs(s - np.sin(exact)) <= dth + 2.0 ** -24).all()
    assert np.array_equal(th[0], np.zeros(hd // 2)) and np.array_equal(th[:, 0], np.arange(n))


def test_attn_ref_without_rounding_points_is_the_model_references_attention_block():
    """q, k rotated by f64ref._rope, then per head softmax(q K^T / sqrt(hd)) V as LlamaF64.eval spells it, against attn_ref(fp16_points = False) -- and rope_ref on the
    exact angles against f64ref._rope."""
    rng = np.random.default_rng(5)
    H, hd, n_past, N = 3, 32, 6, 4
    E, T = H * hd, n_past + N
    x = rng.standard_normal((T, E))
    q = f64ref._rope(rng.standard_normal((N, E)), n_past, H)
    k = f64ref._rope(x, 0, H)
    v = rng.standard_normal((T, E))
    qh, kh, vh = q.reshape(N, H, hd).transpose(1, 0, 2), k.reshape(T, H, hd).transpose(1, 0, 2), v.reshape(T, H, hd).transpose(1, 0, 2)
    s = qh @ kh.transpose(0, 2, 1) / np.sqrt(hd)
    mask = np.arange(T)[None, :] > (n_past + np.arange(N))[:, None]
    want = (f64ref._softmax(np.where(mask[None], -np.inf, s)) @ vh).transpose(1, 0, 2).reshape(N, E)
    for t in range(N):
        for h in range(H):
            out, p, _ = A.attn_ref(qh[h, t], kh[h, :n_past + t + 1], vh[h, :n_past + t + 1], hd, fp16_points=False)
            assert np.abs(out - want[t, h * hd:(h + 1) * hd]).max() <= 1e-12 and abs(p.sum() - 1.0) <= 1e-12
    exact = A.rope_angles_exact(T, hd)
    x32 = x.astype(np.float32)
    assert np.abs(A.rope_ref(x32, np.arange(T), H, (np.cos(exact), np.sin(exact))) - f64ref._rope(x32.astype(np.float64), 0, H)).max() <= 1e-12
    assert np.abs(A.rope_ref(A.rope_unrotate(x, np.arange(T), H, hd), np.arange(T), H, A.rope_tables_ref(T, hd)) - x).max() <= 1e-5   # the inputs' builder inverts it


def test_case_lists_hold_what_the_kernels_change_behaviour_at():
    for hd in A.HDS:
        P = A.body_P(hd)
        assert P == 512 // (hd // 8) and A.BODY_CTX[hd] >= 24 * P + 3 + 8
        assert A.body_positions(hd) == (0, 1, P - 1, P, P + 1, 16 * P - 1, 16 * P, 16 * P + 1, 24 * P + 3)
        assert [c for c in A.VERIFY_CASES if c[0] == hd][:3] == [(hd, 16 * P - 3, R) for R in (1, 2, 8)]
        for S in A.SPLITS:
            Ps, pos = A.split_P(hd), A.split_positions(hd, S)
            n_ctx = A.split_ctx(hd, S)
            assert pos[-1] == n_ctx - 2 and max(pos[:-1]) + 3 <= n_ctx
            a, b, c = pos[7:10]                                       # the last split's range: 16 P - 1, 16 P and 16 P + 1 keys for the score launch
            for T, want in ((a, 16 * Ps - 1), (b, 16 * Ps), (c, 16 * Ps + 1)):
                per = A.split_per(T, S, Ps)
                assert T - (S - 1) * per == want, (hd, S, T)
    assert {c[0] for c in A.DECODE_CASES} == {"one", "batched", "one_own_lead"}
    assert sorted({p for c in A.DECODE_CASES if c[0] == "batched" and c[1] == 128 for p in c[2]}) == sorted(A.body_positions(128))
    assert {s[2] for s in A.ROPE_SEGS} >= {0, 2043} and any(p0 <= 1 < p0 + r for _, r, p0 in A.ROPE_SEGS) and any(p0 + r == A.ROPE_CTX for _, r, p0 in A.ROPE_SEGS)


def test_the_test_library_still_has_the_hooks_the_gpu_tests_use():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "minigpt4.cpp_amd", "csrc", "test_hooks.cpp")).read()
    test = open(os.path.join(root, "include", "minigpt4_amd_test.h")).read()
    pub = open(os.path.join(root, "include", "minigpt4_amd.h")).read()
    for hook in ("minigpt4_amd_test_attn_vsplit(", "minigpt4_amd_test_attn_rows(", "minigpt4_amd_test_attn_prefill_seg(", "minigpt4_amd_test_rope_kv_seg("):
        assert "int " + hook in src and hook in test and hook not in pub, hook
    body = src[src.index("int minigpt4_amd_test_attn_rows("):src.index("int minigpt4_amd_test_ngram_draft(")]
    for call in ("launch_attn_llm_split(", "launch_rope_kv(", "launch_attn_llm(", "attn_split_workspace_bytes(", "hipMemset(dout.p, 0xFF"):
        assert call in body, call
    assert "false, nullptr);" in body                                   # the plain form: fused = false
    from minigpt4_cpp_amd import minigpt4_library as ML
    assert callable(getattr(ML.MiniGPT4SharedLibrary, "amd_test_attn_rows"))
