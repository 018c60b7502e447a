"""Scoring given tokens (minigpt4_amd_score_tokens / _score_batch, k_logprob_rows): the log-probability the model gave every token of a prompt, from the prompt pass
that evaluates it.

  1. the kernel against float64 numpy on the shapes and rows at which it can go wrong;
  2. parity mode against the CPU oracle's all_logits rows, bit for bit;
  3. fast mode against the same rows inside the project's north_star bound;
  4. the conversation afterwards is bit-identical to amd_eval_tokens + amd_logits of the same tokens;
  5. every entry against the engine's own one-pass-per-prefix evaluation;
  6. the 13B width with the real vocabulary (32001: rows not 16-byte aligned, F16 output matrix);
  7. score_batch against score_tokens per conversation and against prefill_batch's state;
  8. refusals leave everything untouched.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOKS = [1, 5, 300, 44, 270, 99, 400, 17, 33, 260, 301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311]   # the 21 tokens of tests/test_gpu_paritymode.py
TOKS70 = TOKS + list(range(312, 361))                                                                       # 70 tokens: one chunk at n_batch = 128, two tiles (64 + 5 target rows)
FILES = [("q5_k", "q5_k_m"), ("q4_0", "none"), ("f16", "none")]
BAR = 1e-2                  # north_star: fast-mode logits within 1e-2 relative
KERNEL_TOL = 1e-4           # |logit| <= 300: one fp32 rounding of x - max (2^-24 * 600 = 3.6e-5) + the sum's ~140 roundings and exp's few ulp after the logarithm (~1e-5), doubled


def _log_softmax64(rows):
    x = np.asarray(rows, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _expected(rows, targets):
    """(logprob, greedy, greedy_logprob) in float64 from logits rows and the ids they predict (-1: none -> logprob 0)."""
    ls = _log_softmax64(rows)
    gr = np.asarray(rows).argmax(axis=-1)                                     # numpy's argmax takes the first maximum too
    t = np.asarray(targets)
    lp = np.where(t >= 0, ls[np.arange(len(t)), np.maximum(t, 0)], 0.0)
    return lp, gr.astype(np.int32), ls[np.arange(len(t)), gr]


# ------------------------------------------------------------------------------------------------ 1. the kernel
SHAPES = [(1, 100, 100), (3, 512, 512), (5, 513, 520), (64, 32000, 32000), (65, 32001, 32001)]


def _launch(lib, x, n_vocab, ld, targets):
    """x: [rows][n_vocab]; the stride's padding is filled with a value that would win every maximum if it were read."""
    rows = x.shape[0]
    buf = np.full((rows, ld), 1e9, np.float32)
    buf[:, :n_vocab] = x
    lp, gr, glp, ms = lib.amd_test_logprob_rows(buf, targets, n_vocab=n_vocab)
    want_lp, want_gr, want_glp = _expected(x, targets)
    print("rows %d n_vocab %d ld %d: max |d logprob| %.3g, max |d greedy_logprob| %.3g, %.3f ms" % (rows, n_vocab, ld, np.abs(lp - want_lp).max(), np.abs(glp - want_glp).max(), ms))
    assert np.isfinite(lp).all() and np.isfinite(glp).all()
    assert np.array_equal(gr, want_gr), (gr, want_gr)
    assert np.abs(lp - want_lp).max() <= KERNEL_TOL, float(np.abs(lp - want_lp).max())
    assert np.abs(glp - want_glp).max() <= KERNEL_TOL, float(np.abs(glp - want_glp).max())
    return lp, gr, glp


def _targets(rng, rows, n_vocab):
    t = rng.integers(0, n_vocab, rows).astype(np.int32)
    for r, v in zip(range(rows), (0, n_vocab - 1, -1)):                       # index 0, the last index and "no target" ...
        t[r] = v
    for r, v in zip(range(rows - 1, 2, -1), (-1, 0, n_vocab - 1)):            # ... also at the tile's far end
        t[r] = v
    return t


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d_v%d_ld%d" % s)
def test_logprob_kernel_against_float64(gpu_lib, shape):
    rows, n_vocab, ld = shape
    rng = np.random.default_rng(rows * 7 + n_vocab)
    base = rng.standard_normal((rows, n_vocab)).astype(np.float32)
    for tset in ([_targets(rng, rows, n_vocab)] if rows > 1 else [np.array([v], np.int32) for v in (0, n_vocab - 1, -1)]):
        lp, _, _ = _launch(gpu_lib, 3.0 * base, n_vocab, ld, tset)
        assert (lp[tset < 0] == 0.0).all()
        _launch(gpu_lib, np.clip(30.0 * base, -300, 300), n_vocab, ld, tset)  # exp of the raw value overflows: the maximum must be subtracted
    # one entry at +300, the rest 0, the target on a 0 entry: about -300, never -inf
    x = np.zeros((rows, n_vocab), np.float32)
    hot = (np.arange(rows) * 37 + 5) % n_vocab
    x[np.arange(rows), hot] = 300.0
    t = ((hot + 1 + np.arange(rows)) % n_vocab).astype(np.int32)
    t[t == hot] = (hot[t == hot] + 1) % n_vocab
    lp, gr, glp = _launch(gpu_lib, x, n_vocab, ld, t)
    assert np.array_equal(gr, hot) and (np.abs(lp + 300.0) < 1e-3).all() and (np.abs(glp) < 1e-3).all()
    # all-equal rows: greedy 0, every log-probability -log(n_vocab)
    x = np.repeat(rng.standard_normal((rows, 1)).astype(np.float32) * 5.0, n_vocab, axis=1)
    lp, gr, glp = _launch(gpu_lib, x, n_vocab, ld, t)
    assert (gr == 0).all()
    assert np.abs(lp + np.log(n_vocab)).max() <= KERNEL_TOL and np.abs(glp + np.log(n_vocab)).max() <= KERNEL_TOL
    # the maximum occurs twice: the lower index wins (pairs that straddle the aligned body's head and tail included)
    x = (3.0 * base).copy()
    lo = (np.arange(rows) * 3) % max(n_vocab // 2, 1)
    hi = n_vocab - 1 - (np.arange(rows) % max(n_vocab // 2 - 1, 1))
    x[np.arange(rows), lo] = 50.0
    x[np.arange(rows), hi] = 50.0
    _, gr, _ = _launch(gpu_lib, x, n_vocab, ld, t)
    assert np.array_equal(gr, lo)


# ------------------------------------------------------------------------------------------------ 2. + 3. against the CPU oracle
_ORACLE = {}


def _oracle_rows(lp_path, toks, chunks, n_ctx=96):
    """The oracle's logits after every token of `toks`, evaluated in the given chunks; computed once per (file, tokens) and shared, never changed."""
    key = (lp_path, tuple(toks), tuple(chunks))
    if key not in _ORACLE:
        import refcpu as R
        from minigpt4_cpp_amd import modelgen as G
        o = R.OracleLLM(G.read_llm_file(lp_path), n_ctx=n_ctx)
        out, at = [], 0
        for c in chunks:
            out.append(o.eval_tokens(toks[at:at + c], all_logits=True))
            at += c
        assert at == len(toks)
        rows = np.concatenate(out)
        rows.setflags(write=False)
        _ORACLE[key] = rows
    return _ORACLE[key]


# n_batch = 16 still evaluates the 21 tokens as ONE chunk (the engine's chunks hold max(n_batch, 32) rows), so the third case is the one whose scored rows cross chunk
# boundaries on the device: 70 tokens at n_batch = 32 = chunks of 32 + 32 + 6, every entry behind the first chunk written at a non-zero host offset
CASES = [(16, TOKS, (16, 5)), (128, TOKS70, (70,)), (32, TOKS70, (32, 32, 6))]
CASE_IDS = ["21_tokens", "70_tokens", "70_tokens_3_chunks"]


def _check_no_logits_entry(res):
    assert res["greedy"][0] == -1 and res["logprob"][0] == 0.0 and res["greedy_logprob"][0] == 0.0
    if "logits" in res:
        assert not res["logits"][0].any()


@pytest.mark.parametrize("wtype,mix", FILES)
@pytest.mark.parametrize("n_batch,toks,chunks", CASES, ids=CASE_IDS)
def test_parity_mode_scores_are_the_oracles(gpu_lib, tiny_files, wtype, mix, n_batch, toks, chunks):
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    want = _oracle_rows(lp, toks, chunks)
    n = len(toks)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=n_batch)
    try:
        gpu_lib.amd_set_parity(ctx, True)
        res = gpu_lib.amd_score_tokens(ctx, toks, want_logits=True)
        assert np.array_equal(res["logits"][1:], want[:n - 1])
        assert np.array_equal(gpu_lib.amd_logits(ctx), want[n - 1])
        assert gpu_lib.library.minigpt4_amd_n_past(ctx.ptr) == n
        _check_no_logits_entry(res)
        e_lp, e_gr, e_glp = _expected(want[:n - 1], toks[1:])
        print("parity", wtype, n, "max |d logprob|", float(np.abs(res["logprob"][1:] - e_lp).max()), "max |d greedy_logprob|", float(np.abs(res["greedy_logprob"][1:] - e_glp).max()))
        assert np.array_equal(res["greedy"][1:], e_gr)
        assert np.abs(res["logprob"][1:] - e_lp).max() <= 1e-4
        assert np.abs(res["greedy_logprob"][1:] - e_glp).max() <= 1e-4
    finally:
        gpu_lib.minigpt4_free(ctx)


@pytest.mark.parametrize("wtype,mix", FILES)
@pytest.mark.parametrize("n_batch,toks,chunks", CASES, ids=CASE_IDS)
def test_fast_mode_scores_within_the_logit_bound(gpu_lib, tiny_files, wtype, mix, n_batch, toks, chunks):
    """A log-probability moves by at most twice the largest logit error of its row: |d logprob| <= 2 * 1e-2 * max |oracle logit of the row|; the oracle's top-1 margin on
    these files and tokens is >= 8.8 % of every row's range, so the greedy ids are equal without exception."""
    from conftest import record_observed
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    want = _oracle_rows(lp, toks, chunks)
    n = len(toks)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=n_batch)
    try:
        res = gpu_lib.amd_score_tokens(ctx, toks)
        _check_no_logits_entry(res)
        e_lp, e_gr, e_glp = _expected(want[:n - 1], toks[1:])
        scale = np.abs(want[:n - 1]).max(axis=1)
        rel = max(float((np.abs(res["logprob"][1:] - e_lp) / scale).max()), float((np.abs(res["greedy_logprob"][1:] - e_glp) / scale).max()))
        print("fast", wtype, n, "max |d logprob| / max |logit|", rel)
        record_observed(f"score_tokens_{wtype}", rel)
        assert (np.abs(res["logprob"][1:] - e_lp) <= 2 * BAR * scale).all()
        assert (np.abs(res["greedy_logprob"][1:] - e_glp) <= 2 * BAR * scale).all()
        assert np.array_equal(res["greedy"][1:], e_gr)
        last = gpu_lib.amd_logits(ctx)
        assert np.abs(last - want[n - 1]).max() <= BAR * np.abs(want[n - 1]).max()
    finally:
        gpu_lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 4. state bit-identity
def _same_state(lib, a, b, steps=8):
    assert lib.library.minigpt4_amd_n_past(a.ptr) == lib.library.minigpt4_amd_n_past(b.ptr)
    assert np.array_equal(lib.amd_logits(a), lib.amd_logits(b))
    pa = [lib.minigpt4_end_chat(a, temp=0.0) for _ in range(steps)]
    pb = [lib.minigpt4_end_chat(b, temp=0.0) for _ in range(steps)]
    assert pa == pb
    assert np.array_equal(lib.amd_logits(a), lib.amd_logits(b))


@pytest.mark.parametrize("n_tokens", [12, 33, 61], ids=lambda n: f"{n}_tokens")
def test_state_after_scoring_is_bit_identical_to_eval_tokens(gpu_lib, tiny_files, n_tokens):
    """n_batch = 16 evaluates chunks of 32 rows: 12 tokens are one chunk, 33 end in a one-row chunk without a target (the captured decode step), 61 in a chunk of 29."""
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    prefix, tokens = TOKS70[:9], TOKS70[9:9 + n_tokens]
    a = lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=16)
    b = lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=16)
    try:
        for c in (a, b):
            lib.amd_eval_tokens(c, prefix)
        pre = lib.amd_logits(b).copy()
        assert np.array_equal(lib.amd_logits(a), pre)
        res = lib.amd_score_tokens(a, tokens)
        lib.amd_eval_tokens(b, tokens)
        lib.amd_logits(b)
        e_lp, e_gr, e_glp = _expected(pre[None, :], tokens[:1])
        assert abs(res["logprob"][0] - e_lp[0]) <= 1e-4 and abs(res["greedy_logprob"][0] - e_glp[0]) <= 1e-4 and res["greedy"][0] == e_gr[0]
        _same_state(lib, a, b)
        # the prefix cache on, both conversations at position 0: the score pass neither consults nor captures the store
        for c in (a, b):
            lib.amd_set_prefix_cache(c, 256)
            lib.minigpt4_reset_chat(c)
        before = lib.amd_prefix_cache_info(a)
        res = lib.amd_score_tokens(a, prefix + tokens)
        after = lib.amd_prefix_cache_info(a)
        assert (after["hits"], after["captures"], after["stored_rows"]) == (before["hits"], before["captures"], before["stored_rows"]) == (0, 0, 0)
        _check_no_logits_entry(res)
        lib.amd_eval_tokens(b, prefix + tokens)
        lib.amd_logits(b)
        assert lib.amd_prefix_cache_info(b)["captures"] == 1                  # the plain pass did capture: the two calls differ in exactly that
        _same_state(lib, a, b)
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


# ------------------------------------------------------------------------------------------------ 5. each entry against one pass per prefix
def test_every_entry_against_one_pass_per_prefix(gpu_lib, tiny_files):
    """The K split of the prompt mat-muls depends on the pass size, so a row of a 13-row pass and the last row of an i-row pass differ by summation order: the bar of
    test_gpu_prefill_batch._check_against_single, 2e-3 of the reference row's range, on the logits; twice that on a log-probability."""
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    toks = TOKS[:13]
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=16)
    ref = lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=16)
    try:
        res = lib.amd_score_tokens(ctx, toks, want_logits=True)
        _check_no_logits_entry(res)
        for i in range(1, len(toks)):
            lib.minigpt4_reset_chat(ref)
            lib.amd_eval_tokens(ref, toks[:i])
            row = lib.amd_logits(ref)
            rng = float(row.max() - row.min())
            e_lp, e_gr, e_glp = _expected(row[None, :], [toks[i]])
            d = float(np.abs(res["logits"][i] - row).max())
            print(i, "logits", d / rng, "logprob", abs(res["logprob"][i] - e_lp[0]) / rng)
            assert d <= 2e-3 * rng, (i, d, rng)
            assert abs(res["logprob"][i] - e_lp[0]) <= 2 * 2e-3 * rng, i
            assert abs(res["greedy_logprob"][i] - e_glp[0]) <= 2 * 2e-3 * rng, i
            assert res["greedy"][i] == e_gr[0], i
    finally:
        lib.minigpt4_free(ctx)
        lib.minigpt4_free(ref)


# ------------------------------------------------------------------------------------------------ 6. the 13B width, n_vocab = 32001
FIXED_40 = [(7919 * (i + 3)) % 31000 + 259 for i in range(40)]


def test_13b_width_real_vocabulary(gpu_lib):
    """13b_v32001_l2: an F16 output matrix of 32001 rows -- the scored tile's rows are not 16-byte aligned.  Greedy ids are compared on the rows whose oracle top-1 margin
    exceeds twice the logit bound (at least three quarters of the rows must be such rows)."""
    import os
    import headline as H
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G
    lib = gpu_lib
    vp, lp = H.headline_files("13b_v32001_l2")
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=512, n_batch=512)
    try:
        toks = lib.amd_tokenize(ctx, G.SYSTEM_PROMPT.encode()) + lib.amd_tokenize(ctx, b"Human: <Img>") + FIXED_40
        n = len(toks)
        assert lib.library.minigpt4_amd_n_vocab(ctx.ptr) == 32001 and 64 < n < 512
        res = lib.amd_score_tokens(ctx, toks)
        R.lib(False).orc_set_threads(max(1, min(len(os.sched_getaffinity(0)), 32)))
        want = R.OracleLLM(G.read_llm_file(lp, in_memory=True), n_ctx=512).eval_tokens(toks, all_logits=True)
        _check_no_logits_entry(res)
        e_lp, e_gr, e_glp = _expected(want[:n - 1], toks[1:])
        scale = np.abs(want[:n - 1]).max(axis=1)
        top2 = np.sort(want[:n - 1], axis=1)[:, -2:]
        decided = (top2[:, 1] - top2[:, 0]) > 2 * BAR * scale
        print("13b_v32001_l2: rows", n - 1, "decided", int(decided.sum()), "max |d logprob| / max |logit|", float((np.abs(res["logprob"][1:] - e_lp) / scale).max()))
        assert (np.abs(res["logprob"][1:] - e_lp) <= 2 * BAR * scale).all()
        assert (np.abs(res["greedy_logprob"][1:] - e_glp) <= 2 * BAR * scale).all()
        assert decided.sum() >= (n - 1) * 3 // 4, int(decided.sum())
        assert np.array_equal(res["greedy"][1:][decided], e_gr[decided])
        last = lib.amd_logits(ctx)
        assert np.abs(last - want[n - 1]).max() <= BAR * np.abs(want[n - 1]).max()
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 7. score_batch
QUESTION = "what is the text in the picture?"
CANDS = {"1_4_9": [[301], [302, 44, 270, 99], [17, 33, 260, 400, 5, 310, 311, 312, 313]],                    # the 1-token candidate has no target row in the pass
         "12_15_9": [list(range(320, 332)), list(range(340, 355)), [17, 33, 260, 400, 5, 310, 311, 312, 313]]}   # 36 packed rows: more than one chunk of 32


def _embed(lib, ctx, seeds):
    from minigpt4_cpp_amd import modelgen as G
    return lib.amd_encode_images(ctx, [G.synth_image(s) for s in seeds])


def _image_turn(lib, ctx, slot, emb, q):
    """The reference's image turn on one conversation: system prompt, then minigpt4_begin_chat_image (queued, not evaluated)."""
    import headline as H
    lib.amd_select_conversation(ctx, slot)
    lib.minigpt4_reset_chat(ctx)
    lib.minigpt4_system_prompt(ctx)
    st, keep = H.embedding_struct(emb)
    lib.minigpt4_begin_chat_image(ctx, st, q)
    del keep


def _forked(lib, vp, lp, emb=None, parity=False):
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=512, n_batch=8)
    lib.amd_set_conversations(ctx, 4)
    if emb is None:
        emb = _embed(lib, ctx, [100])[0]
    if parity:
        lib.amd_set_parity(ctx, True)
    _image_turn(lib, ctx, 0, emb, QUESTION)
    lib.amd_fork_conversation(ctx, 0, [1, 2, 3])
    return ctx, emb


def _slot_state(lib, ctx, slot):
    lib.amd_select_conversation(ctx, slot)
    return lib.amd_logits(ctx).copy(), lib.library.minigpt4_amd_n_past(ctx.ptr)


@pytest.mark.parametrize("cands", list(CANDS), ids=list(CANDS))
def test_score_batch_against_score_tokens_and_prefill_batch(gpu_lib, tiny_files, cands):
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    cand = CANDS[cands]
    slots = [1, 2, 3]
    a, emb = _forked(lib, vp, lp)
    b, _ = _forked(lib, vp, lp, emb)
    c, _ = _forked(lib, vp, lp, emb)
    try:
        got = lib.amd_score_batch(a, slots, cand)
        for s, t, g in zip(slots, cand, got):
            lib.amd_select_conversation(b, s)
            w = lib.amd_score_tokens(b, t, want_logits=True)
            lib.amd_select_conversation(b, 0)
            rows = np.concatenate([lib.amd_logits(b)[None, :], w["logits"][1:]])   # entry 0's row: the fork's logits, still conversation 0's
            rng = rows.max(axis=1) - rows.min(axis=1)
            assert len(g["logprob"]) == len(t)
            assert np.array_equal(g["greedy"], w["greedy"]) and (g["greedy"] >= 0).all(), s
            assert (np.abs(g["logprob"] - w["logprob"]) <= 2 * 2e-3 * rng).all(), s
            assert (np.abs(g["greedy_logprob"] - w["greedy_logprob"]) <= 2 * 2e-3 * rng).all(), s
            assert g["logprob"][0] == w["logprob"][0]                            # the same logits row through the same kernel
        for s, t in zip(slots, cand):
            lib.amd_select_conversation(c, s)
            lib.amd_eval_tokens(c, t)
        lib.amd_prefill_batch(c, slots)
        for s in slots:
            (la, na), (lc, nc) = _slot_state(lib, a, s), _slot_state(lib, c, s)
            assert na == nc and np.array_equal(la, lc), s
        assert lib.amd_end_chat_batch(a, slots, temp=0.0) == lib.amd_end_chat_batch(c, slots, temp=0.0)
    finally:
        for x in (a, b, c):
            lib.minigpt4_free(x)


def test_score_batch_parity_mode_equals_score_tokens(gpu_lib, tiny_files):
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    cand = CANDS["1_4_9"]
    slots = [1, 2, 3]
    a, emb = _forked(lib, vp, lp, parity=True)
    b, _ = _forked(lib, vp, lp, emb, parity=True)
    try:
        got = lib.amd_score_batch(a, slots, cand)
        for s, t, g in zip(slots, cand, got):
            lib.amd_select_conversation(b, s)
            w = lib.amd_score_tokens(b, t)
            for k in ("logprob", "greedy", "greedy_logprob"):
                assert np.array_equal(g[k], w[k]), (s, k)
            la, lb = _slot_state(lib, a, s), _slot_state(lib, b, s)
            assert la[1] == lb[1] and np.array_equal(la[0], lb[0])
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


def test_entry_zero_follows_whether_the_conversation_holds_logits(gpu_lib, tiny_files):
    """No current logits: nothing evaluated yet, after minigpt4_reset_chat, after a partial fork.  Current logits: after any evaluation, after a whole fork."""
    lib = gpu_lib
    vp, llm = tiny_files
    ctx = lib.minigpt4_model_load(vp, llm("q5_k", "q5_k_m", conditioned=True), verbosity=0, n_ctx=96, n_batch=16)
    try:
        lib.amd_set_conversations(ctx, 3)
        _check_no_logits_entry(lib.amd_score_tokens(ctx, TOKS[:6], want_logits=True))       # a fresh conversation
        src = lib.amd_logits(ctx).copy()
        lib.amd_fork_conversation(ctx, 0, [1], n_rows=4)                                     # a prefix only: no logits travel
        lib.amd_fork_conversation(ctx, 0, [2])                                               # the whole state
        lib.amd_select_conversation(ctx, 1)
        _check_no_logits_entry(lib.amd_score_tokens(ctx, TOKS[4:8], want_logits=True))
        lib.amd_select_conversation(ctx, 2)
        res = lib.amd_score_tokens(ctx, TOKS[6:9], want_logits=True)
        e_lp, e_gr, e_glp = _expected(src[None, :], [TOKS[6]])
        assert np.array_equal(res["logits"][0], src) and res["greedy"][0] == e_gr[0] and abs(res["logprob"][0] - e_lp[0]) <= 1e-4 and abs(res["greedy_logprob"][0] - e_glp[0]) <= 1e-4
        lib.minigpt4_reset_chat(ctx)
        _check_no_logits_entry(lib.amd_score_tokens(ctx, TOKS[:3], want_logits=True))
        res = lib.amd_score_batch(ctx, [0, 1], [[5, 6], [7]])                                # conversation 0 holds logits, conversation 1 too (it was scored above)
        assert res[0]["greedy"][0] >= 0 and res[1]["greedy"][0] >= 0
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_everything_untouched(gpu_lib, tiny_files):
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=64, n_batch=16)
    try:
        lib.amd_set_conversations(ctx, 2)
        for s in (0, 1):
            lib.amd_select_conversation(ctx, s)
            lib.amd_eval_tokens(ctx, TOKS[:10 + s])
        before = [_slot_state(lib, ctx, s) for s in (0, 1)]
        lib.amd_select_conversation(ctx, 0)
        V = lib.library.minigpt4_amd_n_vocab(ctx.ptr)

        def untouched():
            for s in (0, 1):
                l, n = _slot_state(lib, ctx, s)
                assert n == before[s][1] and np.array_equal(l, before[s][0]), s
            lib.amd_select_conversation(ctx, 0)

        for bad in ([5, V, 7], [5, -1, 7], [], list(range(3, 3 + 64 - 10 + 1))):   # an id of n_vocab, of -1, n = 0, one token more than fits n_ctx (shift policy off)
            with pytest.raises(RuntimeError, match="score_tokens"):
                lib.amd_score_tokens(ctx, bad)
            untouched()
        good = [[5, 6, 7], [8, 9]]
        for sl, tl in (([0, 0], good), ([0, 2], good), ([-1, 1], good), ([0, 1], [[5, 6], []]), ([0, 1], [[5, V], [6]]), ([0, 1], [[5], [6, -1]]),
                       ([0, 1], [[5], list(range(3, 3 + 64 - 11 + 1))])):          # duplicate, out of range (twice), a count of 0, bad ids, an overflow in the second conversation
            with pytest.raises(RuntimeError, match="score_batch"):
                lib.amd_score_batch(ctx, sl, tl)
            untouched()
        res = lib.amd_score_batch(ctx, [0, 1], good)                               # and the context still works
        assert [len(r["logprob"]) for r in res] == [3, 2] and all((r["greedy"] >= 0).all() for r in res)
        assert [_slot_state(lib, ctx, s)[1] for s in (0, 1)] == [13, 13]
    finally:
        lib.minigpt4_free(ctx)
