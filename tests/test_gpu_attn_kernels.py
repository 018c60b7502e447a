"""Each attention and RoPE / append kernel of the language model ALONE against the float64 reference of tests/attn_ref.py: one launch per case through a test hook, every
output element inside attn_bound (rotated rows and appended keys: rope_bound), appended values bit for bit fp16(v), every cache row the launch does not own unchanged.
The bounds are derived in attn_ref from the kernels' documented rounding points and checked without a GPU by tests/test_cpu_attn_ref.py, on these very cases: fp32
arithmetic in three orders stays inside them, and every wrong variant listed there (a key dropped or counted twice at a boundary, a causal range off by one, a stale row, the
neighbouring RoPE position, ...) is at least 8 bounds away.  Nothing here is tuned to what the kernels give.

  k_attn_llm<hd, fused> / <hd, fused, batched> / k_attn_llm_draft    amd_test_attn_vsplit, VS = 1, forms 0 / 1 / 2
  k_attn_split_scores + k_attn_split_pv                              amd_test_attn_rows mode 0: L steps on ONE workspace (arrival counters zeroed once)
  k_attn_llm<hd, plain> after k_rope_kv                              amd_test_attn_rows mode 1
  k_attn_prefill_h8 / _h<QS 2> / _h<QS 1> / k_attn_prefill           amd_test_attn_prefill_seg, one segment, its per-segment side, forms 1 / 2 / 3 / 4
  k_rope_kv(_slabs) / k_rope_kv_seg(_slabs)                          amd_test_rope_kv_seg, both sides
The largest |got - ref| / bound of each family is printed at the end of the module (pytest -s shows it)."""
import json

import numpy as np
import pytest

import attn_ref as A

pytestmark = pytest.mark.gpu

H = A.N_HEAD
_OBSERVED = {}


@pytest.fixture(scope="module", autouse=True)
def _report_observed():
    yield
    if _OBSERVED:
        print("\nlargest |got - ref| / bound per kernel family:", json.dumps(_OBSERVED, indent=1, sort_keys=True))


def _inside(family, tag, got, want, bound):
    r = A.ratio(got, want, bound)
    _OBSERVED[family] = max(_OBSERVED.get(family, 0.0), r if np.isfinite(r) else 1e30)
    print(f"{family} {tag}: |got - ref| / bound = {r:.3f}")
    assert r <= 1.0, (family, tag, r)


def _u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _check_pass(family, tag, case, ref, out, kc, vc, q_rot=None):
    """out, the appended rows and the rest of the caches of a "pass" launch; kc / vc [n_slot][n_ctx][E] uint16 as the hook returned them"""
    hd, E = case["hd"], case["n_head"] * case["hd"]
    assert out.shape == ref["out"].shape
    _inside(family, tag, out, ref["out"], ref["bound"])
    tabs = A.rope_tables_ref(case["n_ctx"], hd)
    if q_rot is not None:
        _inside(family + " rotated q", tag, q_rot, ref["q_rot"], A.rope_bound(case["q"], case["pos"], hd))
    k_new = np.stack([kc[s, p] for s, p in zip(case["slot"], case["pos"])]).view(np.float16)
    v_new = np.stack([vc[s, p] for s, p in zip(case["slot"], case["pos"])])
    _inside(family + " appended k", tag, k_new, ref["k_rows"], A.rope_bound(case["k"], case["pos"], hd, cache=True, tables=tabs))
    assert np.array_equal(v_new, _u16(ref["v_rows"])), (family, tag, "appended v is not fp16(v) bit for bit")
    untouched = np.ones(kc.shape[:2], bool)
    untouched[case["slot"], case["pos"]] = False
    assert np.array_equal(kc[untouched], _u16(case["kc"])[untouched]) and np.array_equal(vc[untouched], _u16(case["vc"])[untouched]), (family, tag, "a cache row it does not own")


# ---- a. the decode body, VS = 1 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_contexts_fit_the_kernels(gpu_lib):
    """BODY_CTX is the issue's 1024 / 1664 / 3200: the hook refuses (rc = 1) a context above attn_max_ctx / attn_draft_max_ctx, so a launch at each size shows that it fits
    every form, the verify form included -- no smaller context is substituted anywhere below."""
    for hd in A.HDS:
        case = A.verify_case(hd, 0, 8)
        assert case["n_ctx"] == A.BODY_CTX[hd] == {128: 1024, 64: 1664, 32: 3200}[hd]
        gpu_lib.amd_test_attn_vsplit(2, 1, case["q"], case["k"], case["v"], _u16(case["kc"]), _u16(case["vc"]), H, [0] * 8, [0])


@pytest.mark.parametrize("computed", [0, 1], ids=["table", "computed"])
@pytest.mark.parametrize("key", A.DECODE_CASES, ids=lambda k: f"{k[0]}-hd{k[1]}-" + "_".join(map(str, k[2])))
def test_decode_body_one_row_and_batched(gpu_lib, key, computed):
    """Form 0 at every position where the body changes behaviour (partition boundary P, the end of the 16 P prefetch, a ragged steady round -- the first time head sizes
    64 and 32 enter the steady loop), form 1 with three rows in three slots at three of those positions, and the cases whose own key leads the softmax."""
    case, ref = A.decode_case(*key), A.expected_of(A.decode_case, *key)
    n_slot = case["kc"].shape[0]
    n_past = np.zeros(n_slot, np.int32)
    n_past[case["slot"]] = case["pos"]
    form = 1 if key[0] == "batched" else 0
    out, kc, vc = gpu_lib.amd_test_attn_vsplit(form, 1, case["q"], case["k"], case["v"], _u16(case["kc"]), _u16(case["vc"]), H, list(case["slot"]), list(n_past), computed_exp=bool(computed))
    _check_pass("decode body (k_attn_llm fused / batched)", (key, computed), case, ref, out, kc, vc)


@pytest.mark.parametrize("computed", [0, 1], ids=["table", "computed"])
@pytest.mark.parametrize("key", A.VERIFY_CASES, ids=lambda k: f"hd{k[0]}-p{k[1]}-R{k[2]}")
def test_verify_form(gpu_lib, key, computed):
    """R = 1, 2, 8 rows from p0 = 16 P - 3 (the pass's rows straddle a partition boundary and the end of the prefetch), 8 rows from an empty cache and 8 rows into the
    ragged steady round: row t sees the cache rows [0, p0) and the pass's rows 0 .. t."""
    case, ref = A.verify_case(*key), A.expected_of(A.verify_case, *key)
    R = len(case["pos"])
    out, kc, vc = gpu_lib.amd_test_attn_vsplit(2, 1, case["q"], case["k"], case["v"], _u16(case["kc"]), _u16(case["vc"]), H, [0] * R, [key[1]], computed_exp=bool(computed))
    _check_pass("verify form (k_attn_llm_draft)", (key, computed), case, ref, out, kc, vc)


# ---- b. key-split ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def _run_split(lib, case, S, computed):
    out, _, kc, vc = lib.amd_test_attn_rows(0, case["q"], case["k"], case["v"], _u16(case["kc"][0]), _u16(case["vc"][0]), case["n_head"], int(case["pos"][0]), splits=S,
                                            computed_exp=bool(computed))
    assert (out[-1].view(np.uint32) == 0xFFFFFFFF).all(), "the guard row behind the last step's output was written"
    return out[:-1], kc[None], vc[None]


@pytest.mark.parametrize("computed", [0, 1], ids=["table", "computed"])
@pytest.mark.parametrize("key", A.SPLIT_CASES, ids=lambda k: f"hd{k[0]}-S{k[1]}-p{k[2]}")
def test_key_split_steps_on_one_workspace(gpu_lib, key, computed):
    """L = 3 successive steps (2 from n_ctx - 2) on one workspace whose arrival counters were zeroed once: positions with all splits but the first empty, at the
    partition count P, where the keys per split step up (S P), where the last split's range ends at 16 P - 1 / 16 P / 16 P + 1 keys (the steady loop's first round) and
    at the end of the cache.  Step i + 1 must see the row step i appended, and the counters must be back at zero for it."""
    case, ref = A.split_case(*key), A.expected_of(A.split_case, *key)
    assert len(case["pos"]) == (2 if key[2] == case["n_ctx"] - 2 else 3)
    out, kc, vc = _run_split(gpu_lib, case, key[1], computed)
    _check_pass("key-split (k_attn_split_scores + k_attn_split_pv)", (key, computed), case, ref, out, kc, vc)


@pytest.mark.parametrize("key", [(hd, S, A.split_positions(hd, S)[9]) for hd in A.HDS for S in A.SPLITS], ids=lambda k: f"hd{k[0]}-S{k[1]}-p{k[2]}")
def test_key_split_twice_is_bit_identical(gpu_lib, key):
    case = A.split_case(*key)
    a, b = _run_split(gpu_lib, case, key[1], 1), _run_split(gpu_lib, case, key[1], 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), key


@pytest.mark.parametrize("computed", [0, 1], ids=["table", "computed"])
def test_key_split_at_the_13b_grid(gpu_lib, computed):
    """S = 6 with 40 heads at head size 128: the real grid of 240 workgroups across the XCDs, three steps from position 777."""
    key = A.SPLIT_WIDE
    case, ref = A.split_case(*key), A.expected_of(A.split_case, *key)
    out, kc, vc = _run_split(gpu_lib, case, key[1], computed)
    _check_pass("key-split (k_attn_split_scores + k_attn_split_pv)", (key, computed), case, ref, out, kc, vc)


def test_attn_rows_refuses_bad_arguments_before_a_device_is_touched(gpu_lib):
    case = A.plain_case(64, 0, 5)
    args = (case["q"], case["k"], case["v"], _u16(case["kc"][0]), _u16(case["vc"][0]), H)
    for mode, n_past, splits in ((2, 0, 2), (0, 0, 1), (0, 0, 17), (0, -1, 2), (0, case["n_ctx"] - 4, 2), (1, case["n_ctx"] - 4, 0)):
        with pytest.raises(RuntimeError, match="rc=1"):
            gpu_lib.amd_test_attn_rows(mode, *args, n_past, splits=splits)


# ---- c. the plain form -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("computed", [0, 1], ids=["table", "computed"])
@pytest.mark.parametrize("key", A.PLAIN_CASES, ids=lambda k: f"hd{k[0]}-p{k[1]}-N{k[2]}")
def test_plain_form_after_rope_kv(gpu_lib, key, computed):
    """launch_rope_kv, then k_attn_llm<hd, not fused>: N rows at n_past ..., every key from the cache, causal per row; the rotated q against rope_ref as well."""
    case, ref = A.plain_case(*key), A.expected_of(A.plain_case, *key)
    out, q_rot, kc, vc = gpu_lib.amd_test_attn_rows(1, case["q"], case["k"], case["v"], _u16(case["kc"][0]), _u16(case["vc"][0]), H, key[1], computed_exp=bool(computed))
    assert (out[-1].view(np.uint32) == 0xFFFFFFFF).all(), "the guard row behind the last row's output was written"
    _check_pass("plain form (k_rope_kv + k_attn_llm plain)", (key, computed), case, ref, out[:-1], kc[None], vc[None], q_rot=q_rot)


# ---- d. the prompt kernels -------------------------------------------------------------------------------------------------------------------------------------------------------
PROMPT_REFUSED = []           # (form, hd, pos0, N) a form refuses (the hook's rc = 4): none -- every form takes every shape of the list


@pytest.mark.parametrize("form", A.PROMPT_FORMS, ids=lambda f: {1: "h8", 2: "h_qs2", 3: "h_qs1", 4: "f32"}[f])
@pytest.mark.parametrize("key", A.PROMPT_CASES, ids=lambda k: f"hd{k[0]}-p{k[1]}-N{k[2]}")
def test_prompt_kernels(gpu_lib, key, form):
    """One segment, the per-segment side (launch_attn_prefill) of the hook: N at the edges of the 16- and 32-query tiles, first positions at the 64-key tile edge.  The
    cache holds a needle at position pos0 + N, which no query may see, and ordinary rows behind it."""
    case, ref = A.prompt_case_of(*key), A.expected_of(A.prompt_case_of, *key)
    hd, pos0, N = key
    if (form,) + key in PROMPT_REFUSED:
        with pytest.raises(RuntimeError, match="rc=4"):
            gpu_lib.amd_test_attn_prefill_seg(case["kc"], case["vc"], H, [(0, N, pos0)], case["q"], form)
        return
    out_seg, out_ref, _ = gpu_lib.amd_test_attn_prefill_seg(case["kc"], case["vc"], H, [(0, N, pos0)], case["q"], form)
    fam = {1: "prompt k_attn_prefill_h8", 2: "prompt k_attn_prefill_h<QS 2>", 3: "prompt k_attn_prefill_h<QS 1>", 4: "prompt k_attn_prefill (f32)"}[form]
    _inside(fam, key, out_ref, ref["out"], ref["bound"])
    _inside(fam + ", segmented launch", key, out_seg, ref["out"], ref["bound"])


# ---- e. RoPE / append ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", A.ROPE_CASES, ids=lambda k: f"hd{k[0]}-ks{k[1]}")
def test_rope_and_append(gpu_lib, key):
    """k_rope_kv per segment and k_rope_kv_seg (ks = 3: their slab forms, which add three copies of q | k | v in fp32 first): positions 0, 1 and n_ctx - 1 = 2047 among
    the rows, two segments in one slot.  Rotated q and appended k against rope_ref within rope_bound, v bit for bit, every other cache row still zero."""
    hd, ks = key
    q, k, v, slot, pos = A.rope_case(hd, H, A.ROPE_SEGS, 600000 + hd)
    if ks > 1:                                                        # what the slab kernels rotate: acc = x; acc += x; acc += x, each sum rounded to fp32
        q, k, v = ((x + x) + x for x in (q, k, v))
        assert q.dtype == np.float32
    tabs = A.rope_tables_ref(A.ROPE_CTX, hd)
    n_slots = 3
    sides = gpu_lib.amd_test_rope_kv_seg(H, A.ROPE_CTX, n_slots, A.ROPE_SEGS, *A.rope_case(hd, H, A.ROPE_SEGS, 600000 + hd)[:3], ks)
    want_q, want_k = A.rope_ref(q, pos, H, tabs), A.rope_ref(k, pos, H, tabs)
    for name, (q_rot, kc, vc) in zip(("k_rope_kv_seg", "k_rope_kv"), sides):
        fam = f"rope {name}" + ("_slabs" if ks > 1 else "")
        _inside(fam + " rotated q", key, q_rot, want_q, A.rope_bound(q, pos, hd))
        _inside(fam + " appended k", key, kc[slot, pos], want_k, A.rope_bound(k, pos, hd, cache=True, tables=tabs))
        assert np.array_equal(_u16(vc[slot, pos]), _u16(A.f16(v))), (fam, "appended v is not fp16(v) bit for bit")
        untouched = np.ones((n_slots, A.ROPE_CTX), bool)
        untouched[slot, pos] = False
        assert not _u16(kc)[untouched].any() and not _u16(vc)[untouched].any(), (fam, "a cache row outside the segments")
