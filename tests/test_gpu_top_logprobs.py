"""Top-N alternatives with log-probabilities (k_topn_rows; minigpt4_amd_top_logprobs / _end_chat_batch_top / _score_tokens_top / _token_piece).

  1. the kernel against numpy on the shapes and rows at which a selection can go wrong (ties across the cut, -0 / +0, winners in the scalar head and tail);
  2. parity mode against the CPU oracle's all_logits rows;
  3. fast mode against the engine's own logits rows, and the conversation afterwards against plain scoring;
  4. amd_top_logprobs on conversations in three different states, and that it moves nothing;
  5. amd_end_chat_batch_top against a twin context's amd_end_chat_batch;
  6. refusals leave everything untouched;
  7. the server's logprobs keyword.

The selection works on the fp32 inputs themselves: ids and ranks are compared exactly.  Log-probabilities: within KERNEL_TOL of float64, and bit for bit what
k_logprob_rows reports for the same token of the same row.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOKS = [1, 5, 300, 44, 270, 99, 400, 17, 33, 260, 301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311]   # the 21 tokens of tests/test_gpu_score.py
TOKS70 = TOKS + list(range(312, 361))                                                                       # 70 tokens: one chunk at n_batch = 128, two tiles (64 + 5 target rows)
FILES = [("q5_k", "q5_k_m"), ("q4_0", "none"), ("f16", "none")]
KERNEL_TOL = 1e-4           # |logit| <= 300: derived in tests/test_gpu_score.py


def _log_softmax64(rows):
    x = np.asarray(rows, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _order(row, top_n):
    """The first top_n ids in the order 'logit descending, equal logits by ascending id' (-0.0 and +0.0 compare equal)."""
    return np.lexsort((np.arange(len(row)), -row))[:top_n].astype(np.int32)


def _rank(row, t):
    if t < 0:
        return -1
    return int((row > row[t]).sum() + ((row == row[t]) & (np.arange(len(row)) < t)).sum())


def _expected(rows, targets, top_n):
    """(ids [R][top_n], logprobs64 [R][top_n], rank [R], target_logprob64 [R]) from logits rows and one target per row (-1: none)."""
    rows = np.asarray(rows, np.float32)
    ls = _log_softmax64(rows)
    ids = np.stack([_order(r, top_n) for r in rows])
    t = np.asarray(targets)
    rk = np.array([_rank(r, int(v)) for r, v in zip(rows, t)], np.int32)
    tlp = np.where(t >= 0, ls[np.arange(len(t)), np.maximum(t, 0)], 0.0)
    return ids, np.take_along_axis(ls, ids.astype(np.int64), axis=1), rk, tlp


def _check_rows(got_ids, got_lps, got_rank, got_tlp, rows, targets, top_n, tol=KERNEL_TOL):
    ids, lps, rk, tlp = _expected(rows, targets, top_n)
    assert np.array_equal(got_ids, ids), (got_ids, ids)
    assert np.array_equal(got_rank, rk), (got_rank, rk)
    assert np.isfinite(got_lps).all()
    d = max(float(np.abs(got_lps - lps).max()), float(np.abs(got_tlp - tlp).max()))
    assert d <= tol, d
    return d


# ------------------------------------------------------------------------------------------------ 1. the kernel
SHAPES = [(1, 100, 100), (3, 512, 512), (5, 513, 520), (2, 64, 72), (64, 32000, 32000), (65, 32001, 32001)]
TOP_NS = [1, 5, 64]


def _targets(rng, rows, n_vocab):
    t = rng.integers(0, n_vocab, rows).astype(np.int32)
    for r, v in zip(range(rows), (0, n_vocab - 1, -1)):                       # index 0, the last index and "no target" ...
        t[r] = v
    for r, v in zip(range(rows - 1, 2, -1), (-1, 0, n_vocab - 1)):            # ... also at the tile's far end
        t[r] = v
    return t


def _head_tail(r, n_vocab, ld):
    """Row r of a 16-byte aligned [rows][ld] fp32 buffer: the kernel's scalar head is [0, head), its scalar tail [tail0, n_vocab)."""
    head = min(n_vocab, ((16 - (r * ld * 4) % 16) % 16) // 4)
    return head, head + 4 * ((n_vocab - head) // 4)


def _launch(lib, x, n_vocab, ld, targets, top_n, columns=None, row_index=None, buf_rows=None):
    """x: [rows][n_vocab], the rows in the order they are evaluated; the stride's padding is filled with a value that would win every selection if it were read."""
    rows = x.shape[0]
    buf = np.full((rows if buf_rows is None else buf_rows, ld), 1e9, np.float32)
    if row_index is None:
        buf[:rows, :n_vocab] = x
    else:
        buf[:, :n_vocab] = -7.0
        for r, b in enumerate(row_index):
            buf[b, :n_vocab] = x[r]
    ids, lps, rk, tlp, ms = lib.amd_test_topn_rows(buf, top_n, targets, n_vocab=n_vocab, row_index=row_index)
    d = _check_rows(ids, lps, rk, tlp, x, targets, top_n)
    print("rows %d n_vocab %d ld %d top_n %d: max |d logprob| %.3g, %.3f ms" % (rows, n_vocab, ld, top_n, d, ms))
    assert (tlp[np.asarray(targets) < 0] == 0.0).all()
    # bit for bit what the scoring kernel reports for the same token of the same row
    assert np.array_equal(tlp, _score_in_place(lib, buf, n_vocab, targets, row_index))
    for j in (range(top_n) if columns is None else columns):
        assert np.array_equal(lps[:, j], _score_in_place(lib, buf, n_vocab, ids[:, j], row_index)), j
    return ids, lps, rk, tlp


def _score_in_place(lib, buf, n_vocab, targets, row_index):
    """k_logprob_rows' log-probability of targets[r] on row r, every row read at the address at which k_topn_rows read it.  Which thread adds which element follows
    the row's 16-byte alignment, so the same values at another alignment (a gathered copy of rows of 32001 floats) may sum to a neighbouring float: 'the same row'
    is the row where it lies.  With a row_index the whole buffer is scored, a buffer row listed twice in a second launch."""
    if row_index is None:
        return lib.amd_test_logprob_rows(buf, targets, n_vocab=n_vocab)[0]
    out = np.zeros(len(targets), np.float32)
    pending = list(range(len(targets)))
    while pending:
        bt, owner, later = np.full(buf.shape[0], -1, np.int32), {}, []
        for r in pending:
            b = int(row_index[r])
            if b in owner:
                later.append(r)
            else:
                owner[b] = r
                bt[b] = targets[r]
        ref = lib.amd_test_logprob_rows(buf, bt, n_vocab=n_vocab)[0]
        for b, r in owner.items():
            out[r] = ref[b]
        pending = later
    return out


@pytest.mark.parametrize("top_n", TOP_NS, ids=lambda n: "top%d" % n)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d_v%d_ld%d" % s)
def test_topn_kernel_against_numpy(gpu_lib, shape, top_n):
    rows, n_vocab, ld = shape
    V = n_vocab
    rng = np.random.default_rng(rows * 7 + n_vocab + top_n)
    ends = sorted({0, min(top_n, 64) - 1})                                    # the structured rows: the first and the last column against the scoring kernel
    base = rng.standard_normal((rows, V)).astype(np.float32)
    tsets = [_targets(rng, rows, V)] if rows > 1 else [np.array([v], np.int32) for v in (0, V - 1, -1)]
    for t in tsets:
        _launch(gpu_lib, 3.0 * base, V, ld, t, top_n)
        _launch(gpu_lib, np.clip(30.0 * base, -300, 300), V, ld, t, top_n)
    t = tsets[0]
    # row_index: a permutation with one duplicate into a larger buffer
    perm = rng.permutation(rows + 2)[:rows].astype(np.int32)
    x = 3.0 * base
    if rows > 1:
        perm[rows - 1] = perm[0]
        x = x.copy()
        x[rows - 1] = x[0]
    _launch(gpu_lib, x, V, ld, t, top_n, columns=ends, row_index=perm, buf_rows=rows + 2)
    # all-equal rows: ids 0 .. top_n - 1, rank(t) = t
    x = np.repeat(rng.standard_normal((rows, 1)).astype(np.float32) * 5.0, V, axis=1)
    ids, lps, rk, _ = _launch(gpu_lib, x, V, ld, t, top_n, columns=ends)
    assert np.array_equal(ids, np.tile(np.arange(top_n, dtype=np.int32), (rows, 1)))
    assert np.array_equal(rk, np.where(t >= 0, t, -1))
    assert np.abs(lps + np.log(V)).max() <= KERNEL_TOL
    # 7 distinct levels: the cut falls inside a tie group
    levels = np.array([-4.0, -1.5, -0.25, 0.0, 0.5, 2.0, 3.75], np.float32)
    _launch(gpu_lib, levels[rng.integers(0, 7, (rows, V))], V, ld, t, top_n, columns=ends)
    # top_n + 3 copies of the maximum: index 0, the last index, both sides of the row's aligned head and tail, the rest scattered -> the top_n lowest positions, ascending
    x = (3.0 * base).copy()
    want = np.zeros((rows, top_n), np.int32)
    for r in range(rows):
        head, tail0 = _head_tail(r, V, ld)
        pos = {0, V - 1} | {p for p in (head - 1, head, tail0 - 1, tail0) if 0 <= p < V}
        k = min(top_n + 3, V)
        pos = set(sorted(pos)[:k]) if len(pos) > k else pos
        free = np.setdiff1d(np.arange(V), np.fromiter(pos, int))
        pos |= set(rng.choice(free, k - len(pos), replace=False).tolist())
        x[r, sorted(pos)] = 50.0
        want[r] = sorted(pos)[:top_n]
    ids, _, _, _ = _launch(gpu_lib, x, V, ld, t, top_n, columns=ends)
    assert np.array_equal(ids, want)
    # the largest values are a random mix of -0.0 and +0.0, the rest negative: the zeros tie, ids ascending regardless of sign
    x = -np.abs(3.0 * base) - 1.0
    want = np.zeros((rows, top_n), np.int32)
    for r in range(rows):
        z = np.sort(rng.choice(V, min(top_n + 5, V), replace=False))
        x[r, z] = np.where(rng.integers(0, 2, len(z)) == 1, np.float32(-0.0), np.float32(0.0))
        want[r] = z[:top_n]
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    ids, _, _, _ = _launch(gpu_lib, x, V, ld, t, top_n, columns=ends)
    assert np.array_equal(ids, want)
    # an ascending ramp (the winners sit in the scalar tail) and a descending one
    ramp = np.tile(np.arange(V, dtype=np.float32) * np.float32(0.01) - 150.0, (rows, 1))
    ids, _, _, _ = _launch(gpu_lib, ramp, V, ld, t, top_n, columns=ends)
    assert np.array_equal(ids[0], np.arange(V - 1, V - 1 - top_n, -1))
    ids, _, _, _ = _launch(gpu_lib, ramp[:, ::-1].copy(), V, ld, t, top_n, columns=ends)
    assert np.array_equal(ids[0], np.arange(top_n))


# ------------------------------------------------------------------------------------------------ 2. parity mode against the CPU oracle
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


# (n_batch = 16 evaluates chunks of 32 rows: the 21 tokens are one chunk; 70 tokens at n_batch = 32 are chunks of 32 + 32 + 6)
CASES = [(16, TOKS, (16, 5)), (128, TOKS70, (70,)), (32, TOKS70, (32, 32, 6))]
CASE_IDS = ["21_tokens", "70_tokens", "70_tokens_3_chunks"]
TOP = 5


def _check_no_logits_entry(res):
    assert res["logprob"][0] == 0.0 and res["rank"][0] == -1 and (res["top_ids"][0] == -1).all() and (res["top_logprobs"][0] == 0.0).all()


@pytest.mark.parametrize("wtype,mix", FILES)
@pytest.mark.parametrize("n_batch,toks,chunks", CASES, ids=CASE_IDS)
def test_parity_mode_alternatives_are_the_oracles(gpu_lib, tiny_files, wtype, mix, n_batch, toks, chunks):
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    want = _oracle_rows(lp, toks, chunks)
    n = len(toks)
    ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=96, n_batch=n_batch)
    try:
        gpu_lib.amd_set_parity(ctx, True)
        res = gpu_lib.amd_score_tokens(ctx, toks, top_n=TOP)
        _check_no_logits_entry(res)
        d = _check_rows(res["top_ids"][1:], res["top_logprobs"][1:], res["rank"][1:], res["logprob"][1:], want[:n - 1], toks[1:], TOP, tol=1e-4)
        print("parity", wtype, n, "max |d logprob|", d)
        assert np.array_equal(gpu_lib.amd_logits(ctx), want[n - 1])
        assert gpu_lib.library.minigpt4_amd_n_past(ctx.ptr) == n
    finally:
        gpu_lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 3. fast mode against the engine's own rows
def _same_state(lib, a, b, steps=8):
    assert lib.library.minigpt4_amd_n_past(a.ptr) == lib.library.minigpt4_amd_n_past(b.ptr)
    assert np.array_equal(lib.amd_logits(a), lib.amd_logits(b))
    pa = [lib.minigpt4_end_chat(a, temp=0.0) for _ in range(steps)]
    pb = [lib.minigpt4_end_chat(b, temp=0.0) for _ in range(steps)]
    assert pa == pb
    assert np.array_equal(lib.amd_logits(a), lib.amd_logits(b))


def _fast_mode_case(lib, vp, lp, n_ctx, n_batch, prefix, toks, top_n):
    """Context a: amd_score_tokens(want_logits=True); context b: amd_score_tokens(top_n=...) on the same tokens behind the same prefix."""
    a = lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=n_ctx, n_batch=n_batch)
    b = lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=n_ctx, n_batch=n_batch)
    try:
        first = 1
        if prefix:
            for c in (a, b):
                lib.amd_eval_tokens(c, prefix)
            assert np.array_equal(lib.amd_logits(a), lib.amd_logits(b))
            first = 0
        ra = lib.amd_score_tokens(a, toks, want_logits=True)
        rb = lib.amd_score_tokens(b, toks, top_n=top_n)
        if first:
            _check_no_logits_entry(rb)
        rows, t = ra["logits"][first:], toks[first:]                          # entry 0 with a prefix: the logits from before the call (score_tokens copies them out)
        _check_rows(rb["top_ids"][first:], rb["top_logprobs"][first:], rb["rank"][first:], rb["logprob"][first:], rows, t, top_n)
        assert np.array_equal(rb["logprob"], ra["logprob"])
        assert np.array_equal(rb["top_ids"][first:, 0], ra["greedy"][first:]) and np.array_equal(rb["greedy"], rb["top_ids"][:, 0])
        assert np.array_equal(rb["top_logprobs"][first:, 0], ra["greedy_logprob"][first:])
        hit = rb["top_ids"] == np.asarray(toks, np.int32)[:, None]           # wherever the given token is among the alternatives: the same bits
        assert np.array_equal(rb["top_logprobs"][hit], np.repeat(rb["logprob"][:, None], top_n, axis=1)[hit])
        assert np.array_equal(hit.any(axis=1)[first:], rb["rank"][first:] < top_n)
        _same_state(lib, a, b)
        # fixed tokens need not be among a random model's best five: a token that is (the greedy one of b's current row) makes the check above non-empty
        g = int(np.argmax(lib.amd_logits(b)))
        rc = lib.amd_score_tokens(b, [g, 5], top_n=top_n)
        assert rc["rank"][0] == 0 and rc["top_ids"][0, 0] == g and rc["top_logprobs"][0, 0] == rc["logprob"][0]
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


@pytest.mark.parametrize("prefix", [False, True], ids=["fresh", "behind_a_prefix"])
@pytest.mark.parametrize("n_batch,toks,chunks", CASES, ids=CASE_IDS)
def test_fast_mode_alternatives_are_exact_on_the_engines_rows(gpu_lib, tiny_files, n_batch, toks, chunks, prefix):
    vp, llm = tiny_files
    _fast_mode_case(gpu_lib, vp, llm("q5_k", "q5_k_m", conditioned=True), 96, n_batch, [1, 7, 9, 11] if prefix else [], toks, TOP)


FIXED_40 = [(7919 * (i + 3)) % 31000 + 259 for i in range(40)]


def test_13b_width_real_vocabulary(gpu_lib):
    """13b_v32001_l2: 32001-float rows, not 16-byte aligned from the tile's second row on; the token list of test_gpu_score.py's test of the same name."""
    import headline as H
    from minigpt4_cpp_amd import modelgen as G
    lib = gpu_lib
    vp, lp = H.headline_files("13b_v32001_l2")
    tk = lib.minigpt4_model_load(vp, lp, verbosity=1, n_ctx=512, n_batch=512)
    try:
        toks = lib.amd_tokenize(tk, G.SYSTEM_PROMPT.encode()) + lib.amd_tokenize(tk, b"Human: <Img>") + FIXED_40
        assert lib.library.minigpt4_amd_n_vocab(tk.ptr) == 32001 and 64 < len(toks) < 512
    finally:
        lib.minigpt4_free(tk)
    _fast_mode_case(lib, vp, lp, 512, 512, [], toks, 20)


# ------------------------------------------------------------------------------------------------ 4. amd_top_logprobs
def _slot_state(lib, ctx, slot):
    lib.amd_select_conversation(ctx, slot)
    return lib.amd_logits(ctx).copy(), lib.library.minigpt4_amd_n_past(ctx.ptr)


def _three_states(lib, vp, lp, seed=7):
    """Conversation 0 evaluated, 1 with a queued begin_chat, 2 freshly reset."""
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, seed=seed, n_ctx=128, n_batch=16)
    lib.amd_set_conversations(ctx, 3)
    lib.amd_select_conversation(ctx, 0)
    lib.amd_eval_tokens(ctx, TOKS[:9])
    lib.amd_logits(ctx)
    lib.amd_select_conversation(ctx, 1)
    lib.amd_eval_tokens(ctx, TOKS[:5])
    lib.amd_logits(ctx)
    lib.minigpt4_begin_chat(ctx, "what is it?")                                # queued, not evaluated
    lib.amd_select_conversation(ctx, 2)
    lib.amd_eval_tokens(ctx, TOKS[:4])
    lib.amd_logits(ctx)
    lib.minigpt4_reset_chat(ctx)
    lib.amd_select_conversation(ctx, 0)
    return ctx


def test_top_logprobs_describes_the_next_token_and_moves_nothing(gpu_lib, tiny_files):
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    a, b = _three_states(lib, vp, lp), _three_states(lib, vp, lp)
    try:
        slots, targets = [1, 0, 2], [17, -1, 5]
        got = lib.amd_top_logprobs(a, slots, top_n=7, targets=targets)
        lib.amd_prefill_batch(b, slots)
        rows = np.stack([_slot_state(lib, b, s)[0] for s in slots[:2]])
        lib.amd_select_conversation(b, 0)
        _check_rows(got["top_ids"][:2], got["top_logprobs"][:2], got["rank"][:2], got["logprob"][:2], rows, targets[:2], 7)
        assert (got["top_ids"][2] == -1).all() and (got["top_logprobs"][2] == 0.0).all() and got["rank"][2] == -1 and got["logprob"][2] == 0.0
        assert got["rank"][1] == -1 and got["logprob"][1] == 0.0
        none = lib.amd_top_logprobs(a, slots, top_n=7)                        # no targets at all; and a second call sees the same rows
        assert np.array_equal(none["top_ids"], got["top_ids"]) and np.array_equal(none["top_logprobs"], got["top_logprobs"]) and (none["rank"] == -1).all()
        assert lib.library.minigpt4_amd_n_conversations(a.ptr) == 3
        for s in (0, 1):
            (la, na), (lb, nb) = _slot_state(lib, a, s), _slot_state(lib, b, s)
            assert na == nb and np.array_equal(la, lb), s
        for c in (a, b):                                                       # conversation 2 is empty: give it a row before it is sampled
            lib.amd_select_conversation(c, 2)
            lib.amd_eval_tokens(c, TOKS[:3])
            lib.amd_select_conversation(c, 0)
        pa = [lib.amd_end_chat_batch(a, [0, 1, 2], temp=0.8, top_k=40) for _ in range(6)]
        pb = [lib.amd_end_chat_batch(b, [0, 1, 2], temp=0.8, top_k=40) for _ in range(6)]
        assert pa == pb                                                        # the call consumed no random number and moved nothing
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


# ------------------------------------------------------------------------------------------------ 5. amd_end_chat_batch_top
@pytest.mark.parametrize("temp", [0.0, 0.8], ids=["greedy", "temp0.8_top40"])
@pytest.mark.parametrize("B", [1, 3], ids=lambda b: "B%d" % b)
def test_end_chat_batch_top_against_a_twin_context(gpu_lib, tiny_files, B, temp):
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    ctxs = []
    try:
        for _ in range(2):
            c = lib.minigpt4_model_load(vp, lp, verbosity=0, seed=11, n_ctx=128, n_batch=16)
            ctxs.append(c)
            lib.amd_set_conversations(c, 3)
            for s in range(B):
                lib.amd_select_conversation(c, s)
                lib.amd_eval_tokens(c, TOKS[:6 + 2 * s])
            lib.amd_select_conversation(c, 0)
        a, b = ctxs
        slots = list(range(B))
        for step in range(6):
            lib.amd_prefill_batch(b, slots)
            rows = np.stack([_slot_state(lib, b, s)[0] for s in slots])       # what the twin is about to sample from
            lib.amd_select_conversation(b, 0)
            want = lib.amd_end_chat_batch(b, slots, temp=temp, top_k=40)
            got = lib.amd_end_chat_batch_top(a, slots, top_n=4, temp=temp, top_k=40)
            assert got["pieces"] == want, step
            assert [lib.amd_token_piece(a, int(i)) for i in got["ids"]] == want
            _check_rows(got["top_ids"], got["top_logprobs"], got["rank"], got["logprob"], rows, got["ids"], 4)
            if temp == 0.0:
                assert (got["rank"] == 0).all() and np.array_equal(got["ids"], got["top_ids"][:, 0])
        for s in slots:
            (la, na), (lb, nb) = _slot_state(lib, a, s), _slot_state(lib, b, s)
            assert na == nb and np.array_equal(la, lb), s
    finally:
        for c in ctxs:
            lib.minigpt4_free(c)


def test_token_piece(gpu_lib, tiny_files):
    lib = gpu_lib
    vp, llm = tiny_files
    ctx = lib.minigpt4_model_load(vp, llm("q5_k", "q5_k_m", conditioned=True), verbosity=0, n_ctx=64, n_batch=16)
    try:
        V = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
        assert lib.amd_token_piece(ctx, 2) == "</s>"
        assert lib.amd_token_piece(ctx, -1) is None and lib.amd_token_piece(ctx, V) is None
        assert all(isinstance(lib.amd_token_piece(ctx, i), str) for i in (0, 1, V - 1))
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_everything_untouched(gpu_lib, tiny_files):
    import ctypes
    lib = gpu_lib
    L = lib.library
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=64, n_batch=16)
    I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    try:
        lib.amd_set_conversations(ctx, 2)
        for s in (0, 1):
            lib.amd_select_conversation(ctx, s)
            lib.amd_eval_tokens(ctx, TOKS[:10 + s])
        before = [_slot_state(lib, ctx, s) for s in (0, 1)]
        lib.amd_select_conversation(ctx, 0)
        V = L.minigpt4_amd_n_vocab(ctx.ptr)

        def untouched():
            for s in (0, 1):
                l, n = _slot_state(lib, ctx, s)
                assert n == before[s][1] and np.array_equal(l, before[s][0]), s
            lib.amd_select_conversation(ctx, 0)

        for top_n in (0, 65):
            if top_n:                                                          # (the Python layer's top_n = 0 is plain scoring: the C entry point's refusal is below)
                with pytest.raises(RuntimeError, match="score_tokens_top: "):
                    lib.amd_score_tokens(ctx, [5, 6, 7], top_n=top_n)
            with pytest.raises(RuntimeError, match="top_logprobs: "):
                lib.amd_top_logprobs(ctx, [0, 1], top_n=top_n)
            with pytest.raises(RuntimeError, match="end_chat_batch_top: "):
                lib.amd_end_chat_batch_top(ctx, [0, 1], top_n=top_n, temp=0.0)
            untouched()
        # the C entry points themselves: top_n = 0, NULL outputs
        tok, sl = np.array([5, 6, 7], np.int32), np.array([0, 1], np.int32)
        lpv, rk, ids = np.zeros(3, np.float32), np.zeros(3, np.int32), np.zeros(3, np.int32)
        ti, tl = np.zeros((3, 4), np.int32), np.zeros((3, 4), np.float32)
        pieces = (ctypes.c_char_p * 2)()
        ip, fp = (lambda a: None if a is None else a.ctypes.data_as(I32P)), (lambda a: None if a is None else a.ctypes.data_as(F32P))

        def refused(rc, name):
            assert rc == 1 and L.minigpt4_amd_last_error().startswith(name.encode() + b": "), (rc, L.minigpt4_amd_last_error())
            untouched()
        refused(L.minigpt4_amd_score_tokens_top(ctx.ptr, ip(tok), 3, 0, fp(lpv), ip(rk), ip(ti), fp(tl)), "score_tokens_top")
        for args in ((None, 3, 4, lpv, rk, ti, tl), (tok, 3, 4, None, rk, ti, tl), (tok, 3, 4, lpv, None, ti, tl), (tok, 3, 4, lpv, rk, None, tl), (tok, 3, 4, lpv, rk, ti, None),
                     (tok, 0, 4, lpv, rk, ti, tl)):
            t, n, k, p, r, i, l = args
            refused(L.minigpt4_amd_score_tokens_top(ctx.ptr, ip(t), n, k, fp(p), ip(r), ip(i), fp(l)), "score_tokens_top")
        for args in ((None, 2, ti, tl), (sl, 2, None, tl), (sl, 2, ti, None), (sl, 0, ti, tl), (sl, 3, ti, tl)):
            s, n, i, l = args
            refused(L.minigpt4_amd_top_logprobs(ctx.ptr, ip(s), n, 4, None, ip(i), fp(l), None, None), "top_logprobs")
        for args in ((None, ids, lpv, rk, ti, tl), (sl, None, lpv, rk, ti, tl), (sl, ids, None, rk, ti, tl), (sl, ids, lpv, None, ti, tl), (sl, ids, lpv, rk, None, tl),
                     (sl, ids, lpv, rk, ti, None)):
            s, i_, p, r, i, l = args
            refused(L.minigpt4_amd_end_chat_batch_top(ctx.ptr, ip(s), 2, pieces, 0.0, 40, 0.9, 1.0, 1.0, 0, 5.0, 1.0, 4, ip(i_), fp(p), ip(r), ip(i), fp(l)), "end_chat_batch_top")
        refused(L.minigpt4_amd_end_chat_batch_top(ctx.ptr, ip(sl), 2, None, 0.0, 40, 0.9, 1.0, 1.0, 0, 5.0, 1.0, 4, ip(ids), fp(lpv), ip(rk), ip(ti), fp(tl)), "end_chat_batch_top")
        # slot lists: out of range, duplicate
        for bad in ([0, 2], [-1, 1], [0, 0]):
            with pytest.raises(RuntimeError, match="top_logprobs: "):
                lib.amd_top_logprobs(ctx, bad, top_n=3)
            with pytest.raises(RuntimeError, match="end_chat_batch_top: "):
                lib.amd_end_chat_batch_top(ctx, bad, top_n=3, temp=0.0)
            untouched()
        # ids outside the vocabulary; tokens that overflow n_ctx (shift policy off)
        for bad in ([5, V, 7], [5, -1, 7], list(range(3, 3 + 64 - 10 + 1))):
            with pytest.raises(RuntimeError, match="score_tokens_top: "):
                lib.amd_score_tokens(ctx, bad, top_n=3)
            untouched()
        for bad in ([V, -1], [0, -2]):
            with pytest.raises(RuntimeError, match="top_logprobs: "):
                lib.amd_top_logprobs(ctx, [0, 1], top_n=3, targets=bad)
            untouched()
        # and the context still works
        res = lib.amd_score_tokens(ctx, [5, 6, 7], top_n=3)
        assert res["top_ids"].shape == (3, 3) and (res["top_ids"] >= 0).all() and (res["rank"] >= 0).all()
        assert _slot_state(lib, ctx, 0)[1] == 13
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 7. the server
@pytest.mark.parametrize("temp", [0.0, 0.8], ids=["greedy", "temp0.8"])
def test_server_logprobs_keyword(gpu_lib, tiny_files, temp):
    from minigpt4_cpp_amd import modelgen as G
    from minigpt4_cpp_amd import serve as S
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    reqs = [S.Request(G.synth_image(3 + i), p, 6) for i, p in enumerate(["what is the text in the picture?", "describe it", "colour?"])]
    out = []
    for logprobs in (0, 3):
        srv = S.ReplicaServer(vp, lp, conversations=2, n_ctx=1024, n_batch=64, seed=5, library=gpu_lib)   # 3 requests, 2 conversations: waves of 2 + 1
        try:
            out.append(srv.run(reqs, temp=temp, top_k=40, ignore_eos=True, logprobs=logprobs))
            lps = srv.last_logprobs
        finally:
            srv.close()
        if not logprobs:
            assert lps is None
    assert out[0] == out[1]
    assert [len(e) for e in lps] == [6, 6, 6]
    for i, entries in enumerate(lps):
        assert "".join(e["piece"] for e in entries) == out[1][i]              # ignore_eos: every piece is shown
        for e in entries:
            assert len(e["top"]) == 3 and e["rank"] >= 0 and e["logprob"] <= 0.0 and e["top"][0][1] >= e["top"][1][1] >= e["top"][2][1]
            if e["rank"] < 3:
                assert e["top"][e["rank"]] == (e["piece"], e["logprob"])
            if temp == 0.0:
                assert e["top"][0][0] == e["piece"] and e["rank"] == 0 and e["top"][0][1] == e["logprob"]
