"""Guided decoding (classifier-free guidance) on the device: k_guide_rows alone against a float64 reference and its exact properties, then minigpt4_amd_guided_logits and
minigpt4_amd_end_chat_guided on tiny model files against the same rule driven through public calls, then the server.

The float64 reference: M = Lg + s (Lb - Lg) from float64 log-softmax.  Tolerance tol(s) = (1 + 2 |s|) * 2e-4 for |logit| <= 300: lb and lg are each within KERNEL_TOL = 1e-4
(derived in tests/test_gpu_score.py), which contributes (|1 - s| + |s|) * 1e-4 <= (1 + 2 |s|) * 1e-4; the three further fp32 roundings (d, t, m) at magnitudes up to
611 + 1222 |s| add at most 2^-24 of that each, ~ (1 + 2 |s|) * 1.1e-4 together.  Picks are compared exactly; every case asserts that the float64 margin between the best and the
second of M exceeds 4 tol(s), so that no rounding inside the tolerance can change the pick (if a seed ever fails that assertion: change the seed, not the cap)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOKS = [1, 5, 300, 44, 270, 99, 400, 17, 33, 260, 301, 302, 303, 304, 305, 306, 307, 308, 309, 310, 311]
FILES = [("q5_k", "q5_k_m"), ("q4_0", "none"), ("f16", "none")]
SCALES = [-1.0, 0.0, 0.5, 1.0, 1.5, 7.5]
I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


def tol(s):
    return (1.0 + 2.0 * abs(float(s))) * 2e-4


def lsm64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def mix64(b, g, s):
    lb, lg = lsm64(b), lsm64(g)
    return lg + float(s) * (lb - lg)


def margin(m):
    top = np.partition(np.asarray(m, np.float64), -2)[-2:]
    return float(top[1] - top[0])


def first_max(row):
    return int(np.argmax(np.asarray(row) == np.max(row)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_pair(got_m, got_pick, got_val, b, g, s, what):
    """One pair against float64: m within tol(s), the pick exact (the margin is asserted first), the value = m[pick]."""
    want = mix64(b, g, s)
    gap = margin(want)
    err = float(np.abs(got_m.astype(np.float64) - want).max())
    print(f"{what}: scale {s:g} max |m - M| = {err:.3g} (tol {tol(s):.3g}), margin {gap:.3g} = {gap / tol(s):.1f} tol")
    assert gap > 4 * tol(s), (what, gap)
    assert err <= tol(s), (what, err)
    assert int(got_pick) == int(np.argmax(want)), what
    assert bits(got_val) == bits(got_m[int(got_pick)]), what


# ------------------------------------------------------------------------------------------------ 1. the kernel against float64
def pair_table(n, rows):
    """neg before pos in the buffer, one row shared by two pairs, pos == neg, then whatever the row count gives."""
    fixed = [(1, 0), (1, 2), (2, 2)]
    return [fixed[i] if i < 3 and max(fixed[i]) < rows else ((i * 5 + 1) % rows, (i * 7 + 3) % rows) for i in range(n)]


@pytest.mark.parametrize("k,shape", list(enumerate([(1, 100, 100), (3, 513, 520), (2, 64, 72), (4, 32001, 32001), (32, 512, 512)])), ids=lambda v: "p%d_v%d_ld%d" % v if isinstance(v, tuple) else None)
def test_kernel_against_float64(gpu_lib, k, shape):
    n, V, ld = shape
    rows = max(n, 2) + 1
    rng = np.random.default_rng(100 + k)
    buf = np.full((rows, ld), 1e9, np.float32)                                 # the stride padding must never be read
    buf[:, :V] = 3.0 * rng.standard_normal((rows, V)).astype(np.float32)
    pairs = pair_table(n, rows)
    scales = [SCALES[(i + k) % len(SCALES)] for i in range(n)]
    if n >= 6:
        assert set(scales) == set(SCALES)                                      # all six within one launch
    r = gpu_lib.amd_test_guide_rows(buf, pairs, scales, n_vocab=V)
    assert np.isfinite(r["mixed"]).all()
    for i, ((p, g), s) in enumerate(zip(pairs, scales)):
        check_pair(r["mixed"][i], r["pick"][i], r["value"][i], buf[p, :V], buf[g, :V], s, f"pair {i} rows ({p}, {g})")
    again = gpu_lib.amd_test_guide_rows(buf, pairs, scales, n_vocab=V, with_rows=False)   # without the output buffer: the same decision
    assert again["mixed"] is None and np.array_equal(again["pick"], r["pick"]) and np.array_equal(bits(again["value"]), bits(r["value"]))
    assert (r["row_tok"] == -7).all()                                          # no row-token index given: nothing written


def test_all_scales_on_one_pair_of_rows(gpu_lib):
    """Every scale of the list, small shapes included, on rows of a misaligned buffer (ld = 101)."""
    rng = np.random.default_rng(7)
    buf = 3.0 * rng.standard_normal((3, 101)).astype(np.float32)
    pairs = [(2, 1)] * len(SCALES)
    r = gpu_lib.amd_test_guide_rows(buf, pairs, SCALES)
    for i, s in enumerate(SCALES):
        check_pair(r["mixed"][i], r["pick"][i], r["value"][i], buf[2], buf[1], s, f"scale {s:g}")


# ------------------------------------------------------------------------------------------------ 2. exact properties
@pytest.mark.parametrize("V,ld", [(100, 100), (513, 520), (32001, 32001)], ids=lambda v: str(v))
def test_scale_zero_and_equal_rows_are_exact(gpu_lib, V, ld):
    rng = np.random.default_rng(V)
    buf = np.full((4, ld), 1e9, np.float32)
    buf[:, :V] = 3.0 * rng.standard_normal((4, V)).astype(np.float32)
    # scale 0 on (pos, neg) = the pos == neg result on the neg row, whatever that pair's scale
    r = gpu_lib.amd_test_guide_rows(buf, [(3, 1), (1, 1), (1, 1), (2, 1), (1, 1)], [0.0, 1.5, -1.0, 0.0, 0.0], n_vocab=V)
    for i in (0, 2, 3, 4):
        assert np.array_equal(bits(r["mixed"][i]), bits(r["mixed"][1])), i
        assert r["pick"][i] == r["pick"][1] and bits(r["value"][i]) == bits(r["value"][1])
    # pos == neg: the log-probabilities k_topn_rows reports for the same row at the same address, and its first id
    for row in (0, 1, 2, 3):
        e = gpu_lib.amd_test_guide_rows(buf, [(row, row)], [7.5], n_vocab=V)
        ids, lps, _, _, _ = gpu_lib.amd_test_topn_rows(buf, 64, [-1], n_vocab=V, row_index=[row])
        assert np.array_equal(bits(e["mixed"][0][ids[0]]), bits(lps[0])), row
        assert e["pick"][0] == ids[0][0] and bits(e["value"][0]) == bits(lps[0][0])
        want = lsm64(buf[row, :V])
        assert np.abs(e["mixed"][0] - want).max() <= 1e-4


def test_ties_take_the_lower_id(gpu_lib):
    V = ld = 32001                                                             # rows 1 .. 3 start 4, 8 and 12 bytes past a 16-byte boundary
    rng = np.random.default_rng(11)
    base = 3.0 * rng.standard_normal((4, V)).astype(np.float32)
    spans = {}
    for r in range(4):
        head = (-r * ld) % 4
        spans[r] = (head, head + 4 * ((V - head) // 4))                        # the scalar head is [0, head), the scalar tail [tail0, V)
    assert spans[1] == (3, 31999) and spans[2] == (2, 31998) and spans[3] == (1, 32001)   # row 3 has no scalar tail
    for pos in (1, 2, 3):
        head, tail0 = spans[pos]
        group = [(head - 1, head), (0, V - 1), (777, 20001)] + ([(tail0 - 1, tail0), (head, tail0), (tail0, V - 1)] if tail0 < V else [(head, V - 1)])
        neg = (pos + 1) % 4
        for j1, j2 in group:                                                   # one launch per duplicated pair of columns: each needs the rows to itself
            x = base.copy()
            x[pos, [j1, j2]] = 40.0
            x[neg, [j1, j2]] = -5.0                                            # identical column values in both rows: m is the same float at j1 and j2
            r = gpu_lib.amd_test_guide_rows(x, [(pos, neg), (neg, pos)], [1.5, -1.0], n_vocab=V)
            for i in (0, 1):                                                   # pair 1 walks the other row's span
                m = r["mixed"][i]
                assert bits(m[j1]) == bits(m[j2]) and m[j1] == m.max(), (pos, j1, j2, i)
                assert r["pick"][i] == j1 and bits(r["value"][i]) == bits(m[j1]), (pos, j1, j2, i, r["pick"][i])


def test_all_equal_rows_pick_zero(gpu_lib):
    """Constant rows: every m is the same float, so the lowest id, 0, wins -- for every scale (a negative one and 0 included), on every alignment a 32 001-float row takes
    in the buffer, and on a small aligned shape."""
    for V, ld in ((32001, 32001), (100, 104)):
        buf = np.full((5, ld), 1e9, np.float32)
        for r, c in enumerate((2.5, -7.0, 0.0, -0.0, 300.0)):
            buf[r, :V] = c
        pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (1, 1), (3, 3)]      # rows 0 .. 4 start 0, 4, 8, 12 and 0 bytes past a 16-byte boundary when ld = 32001
        for s in SCALES:
            r = gpu_lib.amd_test_guide_rows(buf, pairs, [s] * len(pairs), n_vocab=V)
            assert (r["pick"] == 0).all(), (V, s, r["pick"])
            for i in range(len(pairs)):
                m = r["mixed"][i]
                assert (bits(m) == bits(m[0])).all() and bits(r["value"][i]) == bits(m[0]), (V, s, i)
                assert abs(float(m[0]) + np.log(V)) <= 1e-4                    # log-softmax of a constant row, whatever the scale: lg + s (lb - lg) with lb == lg
            again = gpu_lib.amd_test_guide_rows(buf, pairs, [s] * len(pairs), n_vocab=V, with_rows=False)
            assert (again["pick"] == 0).all() and np.array_equal(bits(again["value"]), bits(r["value"]))


def test_signed_zeros(gpu_lib):
    """The rule says -0 equals +0 in the pick.  Two halves.
    RAW rows whose maxima are -0.0 and +0.0: they are equal logits, so m is the same float at both ids and the lower id wins, whichever of the two carries the sign.
    m ITSELF is never -0 for finite rows, so a -0 / +0 tie between two values of m cannot be produced: lg = (g - max g) - log(sum) is +0 (the maximum's own term when the
    sum is exactly 1: +0 - +0) or negative, never -0, and m = lg + t with t = scale * d is -0 only if both terms are.  The case that comes closest is asserted: a dominant
    logit (every other term underflows, lg = +0 at it) with t = -0 there (scale 0 with d <= 0, a negative scale with d = +0): m must be +0, bit for bit."""
    V = 100
    rng = np.random.default_rng(5)
    buf = (-1.0 - np.abs(3.0 * rng.standard_normal((4, V)))).astype(np.float32)   # everything below zero ...
    buf[0, 3], buf[0, 7] = -0.0, 0.0                                           # ... but the maxima: -0 at the lower id, +0 at the higher
    buf[1] = buf[0]                                                            # the same logits ...
    buf[1, 3], buf[1, 7] = 0.0, -0.0                                           # ... with the signs of the zeros the other way round
    r = gpu_lib.amd_test_guide_rows(buf, [(0, 0), (1, 1), (0, 1), (1, 0)], [1.0, 7.5, 1.5, -1.0])
    for i in (0, 1, 2, 3):
        assert r["pick"][i] == 3 and bits(r["mixed"][i][3]) == bits(r["mixed"][i][7]), i
    # a dominant logit: lg = +0 there
    dom = (3.0 * rng.standard_normal((3, V))).astype(np.float32)
    dom[0, 11] = dom[1, 11] = 300.0                                            # exp(x - 300) underflows to 0 for every other x: both sums are exactly 1
    dom[2, 11] = 250.0
    dom[2, 40] = 300.0                                                         # row 2: dominant elsewhere, so lb[11] < 0 = lg[11] against rows 0 / 1
    pairs, scales = [(0, 1), (0, 1), (0, 1), (2, 1), (2, 1), (0, 0)], [0.0, -1.0, -7.5, 0.0, -0.0, -1.0]
    r = gpu_lib.amd_test_guide_rows(dom, pairs, scales)
    for i in range(len(pairs)):
        m = r["mixed"][i]
        assert bits(m[11]) == 0, (i, m[11], hex(int(bits(m[11]))))            # +0, not -0: lg = +0 and t = -0 (0 * negative, negative * +0)
        assert not (bits(m) == 0x80000000).any(), i                           # and no -0 anywhere in the row
        assert r["pick"][i] == 11 and bits(r["value"][i]) == 0, i
    for i in (3, 4):
        assert mix64(dom[2], dom[1], scales[i])[11] == 0.0


# ------------------------------------------------------------------------------------------------ 3. the row-token hand-off
def test_picks_go_into_exactly_their_row_tokens(gpu_lib):
    rng = np.random.default_rng(3)
    buf = 3.0 * rng.standard_normal((5, 513)).astype(np.float32)
    before = np.arange(64, dtype=np.int32) + 1000
    idx = [(4, 5), (-1, -1), (0, 63), (-1, 9)]
    r = gpu_lib.amd_test_guide_rows(buf, [(0, 1), (2, 3), (4, 0), (3, 3)], [1.5, 1.5, 0.5, 1.0], row_tok_index=idx, row_tok=before)
    want = before.copy()
    for (a, b), p in zip(idx, r["pick"]):
        for j in (a, b):
            if j >= 0:
                want[j] = p
    assert np.array_equal(r["row_tok"], want)
    assert (r["pick"] >= 0).all() and (r["pick"] < 513).all() and (want[[4, 5, 0, 63, 9]] < 513).all()
    assert np.array_equal(np.flatnonzero(r["row_tok"] != before), [0, 4, 5, 9, 63])


# ------------------------------------------------------------------------------------------------ engine helpers
def _state(lib, ctx, slot):
    lib.amd_select_conversation(ctx, slot)
    return lib.amd_logits(ctx).copy(), lib.library.minigpt4_amd_n_past(ctx.ptr)


def _load(lib, vp, lp, prompts, seed=7, n_ctx=128, n_batch=16, extra=0):
    """One conversation per prompt (a token list), evaluated; `extra` more conversations left empty."""
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, seed=seed, n_ctx=n_ctx, n_batch=n_batch)
    lib.amd_set_conversations(ctx, len(prompts) + extra)
    for s, p in enumerate(prompts):
        lib.amd_select_conversation(ctx, s)
        lib.amd_eval_tokens(ctx, p)
        lib.amd_logits(ctx)
    lib.amd_select_conversation(ctx, 0)
    return ctx


PROMPTS = [TOKS[:9], TOKS[4:9], TOKS[2:13], [1, 17, 33], TOKS[:15], [1, 400, 99, 270]]


# ------------------------------------------------------------------------------------------------ 4. amd_guided_logits
@pytest.mark.parametrize("wtype,mix", FILES)
def test_guided_logits_against_float64_and_moves_nothing(gpu_lib, tiny_files, wtype, mix):
    lib = gpu_lib
    L = lib.library
    vp, llm = tiny_files
    lp = llm(wtype, mix, conditioned=True)
    a, b = _load(lib, vp, lp, PROMPTS[:4], extra=1), _load(lib, vp, lp, PROMPTS[:4], extra=1)
    try:
        for c in (a, b):                                                       # conversation 1: rows queued, not evaluated; conversation 4: evaluated, then reset
            lib.amd_select_conversation(c, 1)
            lib.minigpt4_begin_chat(c, "what is it?")
            lib.amd_select_conversation(c, 4)
            lib.amd_eval_tokens(c, TOKS[:4])
            lib.amd_logits(c)
            lib.minigpt4_reset_chat(c)
            lib.amd_select_conversation(c, 0)
        s = 1.5
        got = lib.amd_guided_logits(a, [0, 2], [1, 3], s)
        lib.amd_prefill_batch(b, [0, 1, 2, 3])                                 # the twin: the queued rows, nothing else
        rows = [_state(lib, b, k)[0] for k in range(4)]
        assert lib.library.minigpt4_amd_n_past(b.ptr) > 0
        for i, (p, g) in enumerate([(0, 1), (2, 3)]):
            want = mix64(rows[p], rows[g], s)
            err = float(np.abs(got["mixed"][i] - want).max())
            print(f"{wtype} pair {i}: max |m - M| = {err:.3g} (tol {tol(s):.3g}), margin {margin(want) / tol(s):.1f} tol")
            assert err <= tol(s)
            assert got["pick"][i] == first_max(got["mixed"][i])
            assert margin(want) > 4 * tol(s), (wtype, i, margin(want) / tol(s))   # the conditioned tiny files decide by thousands of tol
            assert got["pick"][i] == int(np.argmax(want))
        only = lib.amd_guided_logits(a, [0, 2], [1, 3], s, with_rows=False)    # NULL mixed_out
        assert only["mixed"] is None and np.array_equal(only["pick"], got["pick"])
        for k in range(4):                                                     # position and logits: those of the twin, which only evaluated its queue
            (la, na), (lb, nb) = _state(lib, a, k), _state(lib, b, k)
            assert na == nb and np.array_equal(la, lb), k
        assert lib.amd_guidance_info(a) == dict(launches=2, handed=0, pen_picked=0, sampled=0)
        assert lib.amd_guidance_info(b) == dict(launches=0, handed=0, pen_picked=0, sampled=0)
        # refusals leave everything untouched
        before = [_state(lib, a, k) for k in range(4)]
        pick = np.zeros(4, np.int32)
        toks = (ctypes.c_char_p * 4)()
        ip = lambda x: np.ascontiguousarray(x, np.int32).ctypes.data_as(I32P)

        def refused(pos, neg, n, scale=1.5, why=b""):
            pa, na_ = np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(neg, np.int32)
            calls = (("guided_logits", lambda: L.minigpt4_amd_guided_logits(a.ptr, pa.ctypes.data_as(I32P), na_.ctypes.data_as(I32P), n, scale, None, ip(pick))),
                     ("end_chat_guided", lambda: L.minigpt4_amd_end_chat_guided(a.ptr, pa.ctypes.data_as(I32P), na_.ctypes.data_as(I32P), n, scale, toks, 0.0, 40, 0.9, 1.0,
                                                                                1.0, 0, 5.0, 1.0, None)))
            for name, call in calls:
                rc = call()
                msg = L.minigpt4_amd_last_error()
                assert rc == 1 and msg.startswith(name.encode() + b": ") and why in msg, (name, rc, msg)
            for k in range(4):
                l, npast = _state(lib, a, k)
                assert npast == before[k][1] and np.array_equal(l, before[k][0]), k
            lib.amd_select_conversation(a, 4)
            assert lib.library.minigpt4_amd_n_past(a.ptr) == 0
            lib.amd_select_conversation(a, 0)
        refused([0, 1], [1, 2], 2, why=b"distinct")                            # a conversation in both lists
        refused([0, 0], [1, 2], 2, why=b"distinct")
        refused([0], [5], 1, why=b"distinct and in range")
        refused([0], [4], 1, why=b"no current logits")                         # after minigpt4_reset_chat
        refused([0, 1, 2], [3, 4, 0], 3)                                       # 2 n above the number of conversations
        refused([0], [1], 0)
        refused([0], [1], 1, scale=float("inf"), why=b"finite")
        refused([0], [1], 1, scale=float("nan"), why=b"finite")
        assert L.minigpt4_amd_guided_logits(a.ptr, None, ip([1]), 1, 1.5, None, ip(pick)) == 1 and L.minigpt4_amd_last_error().startswith(b"guided_logits: ")
        assert lib.amd_guidance_info(a)["launches"] == 2
        # and neither the generator nor anything else moved: both contexts sample the same from here on
        pa = [lib.amd_end_chat_batch(a, [0, 1, 2, 3], temp=0.8, top_k=40) for _ in range(4)]
        pb = [lib.amd_end_chat_batch(b, [0, 1, 2, 3], temp=0.8, top_k=40) for _ in range(4)]
        assert pa == pb
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


# ------------------------------------------------------------------------------------------------ 5. amd_end_chat_guided, greedy, against a twin context
def _twin_step(lib, b, pos, neg, s, what):
    """The rule through public calls: the pick in float64 from the twin's own two rows (margin asserted), both conversations advanced by it with amd_eval_batch."""
    ids = []
    for p, g in zip(pos, neg):
        want = mix64(_state(lib, b, p)[0], _state(lib, b, g)[0], s)
        gap = margin(want)
        assert gap > 4 * tol(s), (what, p, g, gap / tol(s))
        ids.append(int(np.argmax(want)))
    lib.amd_select_conversation(b, 0)
    slots = [x for pg in zip(pos, neg) for x in pg]
    lib.amd_eval_batch(b, slots, [t for t in ids for _ in (0, 1)])
    return ids


@pytest.mark.parametrize("n_pairs,parity", [(1, False), (3, False), (1, True)], ids=["one_pair", "three_pairs", "one_pair_parity_mode"])
def test_end_chat_guided_greedy_equals_the_twin(gpu_lib, tiny_files, n_pairs, parity):
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    prompts = PROMPTS[:2 * n_pairs]
    a, b = _load(lib, vp, lp, prompts), _load(lib, vp, lp, prompts)
    try:
        for c in (a, b):
            lib.amd_set_parity(c, parity)
        if parity:                                                             # the prompts again, in the mode under test
            for c in (a, b):
                for k, p in enumerate(prompts):
                    lib.amd_select_conversation(c, k)
                    lib.minigpt4_reset_chat(c)
                    lib.amd_eval_tokens(c, p)
                    lib.amd_logits(c)
                lib.amd_select_conversation(c, 0)
        pos, neg, s = list(range(0, 2 * n_pairs, 2)), list(range(1, 2 * n_pairs, 2)), 1.5
        for step in range(16):
            want = _twin_step(lib, b, pos, neg, s, f"step {step}")
            pieces, ids = lib.amd_end_chat_guided(a, pos, neg, s, temp=0.0, with_ids=True)
            assert list(ids) == want, step
            assert pieces == [lib.amd_token_piece(a, t) for t in want]
            for k in range(2 * n_pairs):                                       # the same launches and the same graph: the same bits
                (la, na), (lb, nb) = _state(lib, a, k), _state(lib, b, k)
                assert na == nb == len(prompts[k]) + step + 1 and np.array_equal(la, lb), (step, k)
                assert lib.amd_token_history(a)[-1] == want[k // 2]
            lib.amd_select_conversation(a, 0)
        info = lib.amd_guidance_info(a)
        assert info == dict(launches=16, handed=0 if parity else 16 * n_pairs, pen_picked=0, sampled=0)
        assert lib.amd_penalty_info(a)["launches"] == 0 and lib.amd_penalty_info(a)["host_rows"] == 0
        # the greedy and feed tokens are each conversation's own: an ordinary greedy step agrees on both contexts
        slots = list(range(2 * n_pairs))
        assert lib.amd_end_chat_batch(a, slots, temp=0.0) == lib.amd_end_chat_batch(b, slots, temp=0.0)
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


# ------------------------------------------------------------------------------------------------ 6. bias and penalties act on the guided row
def test_bias_and_penalties_act_on_the_guided_row(gpu_lib, tiny_files):
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    s = 1.5
    ctxs = [_load(lib, vp, lp, PROMPTS[:2]) for _ in range(3)]
    try:
        a, b, c = ctxs
        m = lib.amd_guided_logits(a, [0], [1], s)["mixed"][0]
        best = first_max(m)
        rest = m.copy()
        rest[best] = -np.inf
        second = first_max(rest)
        # neg's bias changes nothing: the kernel's pick is handed over
        lib.amd_select_conversation(a, 1)
        lib.amd_set_logit_bias(a, {best: -np.inf})
        lib.amd_select_conversation(a, 0)
        assert list(lib.amd_end_chat_guided(a, [0], [1], s, temp=0.0, with_ids=True)[1]) == [best]
        assert lib.amd_guidance_info(a) == dict(launches=2, handed=1, pen_picked=0, sampled=0)
        # pos's bias bans the guided pick: the second of m
        lib.amd_select_conversation(b, 0)
        lib.amd_set_logit_bias(b, {best: -np.inf})
        assert list(lib.amd_end_chat_guided(b, [0], [1], s, temp=0.0, with_ids=True)[1]) == [second]
        assert lib.amd_guidance_info(b) == dict(launches=1, handed=0, pen_picked=1, sampled=0)
        assert lib.amd_penalty_info(b)["launches"] == 1
        for k in (0, 1):                                                       # both advanced by the token that was picked, and the raw logits stayed raw
            lib.amd_select_conversation(b, k)
            assert lib.amd_token_history(b)[-1] == second
        lib.amd_select_conversation(a, 0)
        # repeat_penalty 1.3 over a window that contains the pick: guided steps until the guided pick is a token of pos's history
        lib.amd_select_conversation(c, 0)
        found = None
        for step in range(40):
            row = lib.amd_guided_logits(c, [0], [1], s)["mixed"][0]
            hist = lib.amd_token_history(c)
            if first_max(row) in set(int(t) for t in hist[-64:]):
                found = step
                break
            lib.amd_end_chat_guided(c, [0], [1], s, temp=0.0)
        assert found is not None, "no guided pick repeated a token of the window in 40 steps: choose other prompts"
        print(f"the guided pick {first_max(row)} is in the window after {found} steps")
        lib.amd_set_penalties(c, True)
        lib.amd_conversation_penalties(c, 0, repeat_last_n=64, repeat_penalty=1.3)
        lib.amd_conversation_penalties(c, 1, repeat_last_n=64, repeat_penalty=5.0, alpha_presence=3.0)   # neg's: ignored
        n_ctx = 128
        want_row = lib.amd_test_penalise_host(row, hist, n_ctx, repeat_last_n=64, repeat_penalty=1.3)[0]
        assert bits(want_row[first_max(row)]) != bits(row[first_max(row)])     # the penalty did touch the pick
        before = lib.amd_guidance_info(c)
        got = int(lib.amd_end_chat_guided(c, [0], [1], s, temp=0.0, with_ids=True)[1][0])
        assert got == first_max(want_row)                                      # exact: both sides start from the same bits
        after = lib.amd_guidance_info(c)
        assert after["pen_picked"] == before["pen_picked"] + 1 and after["handed"] == before["handed"]
        assert lib.amd_penalty_info(c)["launches"] == 1
    finally:
        for x in ctxs:
            lib.minigpt4_free(x)


# ------------------------------------------------------------------------------------------------ 7. the host chain
def _sample(lib, ctx, temp, top_k):
    tid = np.zeros(1, np.int32)
    assert lib.library.minigpt4_amd_sample(ctx.ptr, tid.ctypes.data_as(I32P), temp, top_k, 0.9, 1.0, 1.0, 0, 5.0, 1.0) == 0
    return int(tid[0])


def test_host_chain_samples_the_guided_row(gpu_lib, tiny_files):
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    s = 1.5
    a, b = _load(lib, vp, lp, PROMPTS[:5], seed=21), _load(lib, vp, lp, PROMPTS[:5], seed=21)
    try:
        # top_k 1: whatever is drawn, the chain returns the first maximum of the guided row
        want = lib.amd_guided_logits(a, [0, 2], [1, 3], s)["pick"]
        got = lib.amd_end_chat_guided(a, [0, 2], [1, 3], s, temp=0.8, top_k=1, with_ids=True)[1]
        assert np.array_equal(got, want)
        assert lib.amd_guidance_info(a) == dict(launches=2, handed=0, pen_picked=0, sampled=2)
        for _ in range(2):                                                     # the twin draws twice as well
            _sample(lib, b, 0.8, 1)
        # top_k 40: one call over two pairs advances the generator by exactly two draws
        ids = lib.amd_end_chat_guided(a, [0, 2], [1, 3], s, temp=0.8, top_k=40, with_ids=True)[1]
        assert ((ids >= 0) & (ids < 512)).all()
        for k, t in zip((0, 1, 2, 3), (ids[0], ids[0], ids[1], ids[1])):
            lib.amd_select_conversation(a, k)
            assert lib.amd_token_history(a)[-1] == t
        for _ in range(2):
            _sample(lib, b, 0.8, 40)
        for c in (a, b):
            lib.amd_select_conversation(c, 4)                                  # conversation 4: not in any pair, equal logits in both contexts
        assert np.array_equal(lib.amd_logits(a), lib.amd_logits(b))
        assert [_sample(lib, a, 0.8, 40) for _ in range(6)] == [_sample(lib, b, 0.8, 40) for _ in range(6)]
        assert lib.amd_guidance_info(a)["sampled"] == 4
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


# ------------------------------------------------------------------------------------------------ 8. both or neither
def test_a_pair_advances_both_conversations_or_neither(gpu_lib, tiny_files):
    lib = gpu_lib
    vp, llm = tiny_files
    lp = llm("q5_k", "q5_k_m", conditioned=True)
    rng = np.random.default_rng(2)
    long = [1] + [int(t) for t in rng.integers(3, 512, 63)]
    ctx = _load(lib, vp, lp, [long[:63], long[1:] + [7]], n_ctx=64, n_batch=16)   # pos at 63: one row of room; neg at 64: none
    try:
        assert _state(lib, ctx, 0)[1] == 63 and _state(lib, ctx, 1)[1] == 64
        want = int(lib.amd_guided_logits(ctx, [0], [1], 1.5)["pick"][0])
        ids = lib.amd_end_chat_guided(ctx, [0], [1], 1.5, temp=0.0, with_ids=True)[1]
        assert int(ids[0]) == want                                             # sampled and reported ...
        assert _state(lib, ctx, 0)[1] == 63 and _state(lib, ctx, 1)[1] == 64   # ... and neither moved
        assert lib.amd_guidance_info(ctx)["handed"] == 0
        lib.amd_set_context_shift(ctx, 4)
        ids = lib.amd_end_chat_guided(ctx, [0], [1], 1.5, temp=0.0, with_ids=True)[1]
        assert int(ids[0]) == want                                             # the same logits decided
        assert _state(lib, ctx, 0)[1] == 64                                    # pos had the room
        assert _state(lib, ctx, 1)[1] == 64 - (64 - 4) // 2 + 1                # neg shifted by its own rule, then advanced
        for k in (0, 1):
            lib.amd_select_conversation(ctx, k)
            assert lib.amd_token_history(ctx)[-1] == want
        assert lib.amd_guidance_info(ctx)["handed"] == 1
    finally:
        lib.minigpt4_free(ctx)


# ------------------------------------------------------------------------------------------------ 9. the server
def _manual(lib, ctx, reqs, scale, batched, negative, conversations):
    """ReplicaServer.run(guidance_scale=scale, ignore_eos=True) through the binding: waves of conversations // 2 requests, two conversations each."""
    from minigpt4_cpp_amd import minigpt4_library as ML
    out = []
    per_wave = conversations // 2
    for w in range(0, len(reqs), per_wave):
        wave = reqs[w:w + per_wave]
        for j, r in enumerate(wave):
            emb = lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(r.image))
            lib.amd_select_conversation(ctx, 2 * j)
            lib.minigpt4_reset_chat(ctx)
            lib.minigpt4_system_prompt(ctx)
            lib.minigpt4_begin_chat_image(ctx, emb, r.prompt)
            lib.minigpt4_free_embedding(emb)
            lib.amd_select_conversation(ctx, 2 * j + 1)
            lib.minigpt4_reset_chat(ctx)
            lib.minigpt4_system_prompt(ctx)
            lib.minigpt4_begin_chat(ctx, r.prompt if negative is None else negative)
        if batched:
            lib.amd_prefill_batch(ctx, list(range(2 * len(wave))))
        text = [""] * len(wave)
        left = [r.max_tokens for r in wave]
        active = [j for j in range(len(wave)) if left[j] > 0]
        while active:
            pieces = lib.amd_end_chat_guided(ctx, [2 * j for j in active], [2 * j + 1 for j in active], scale, temp=0.0)
            for j, p in zip(active, pieces):
                text[j] += p
                left[j] -= 1
            active = [j for j in active if left[j] > 0]
        out += text
    lib.amd_select_conversation(ctx, 0)
    return out


def test_server_guidance_keywords(gpu_lib, tmpdir_models):
    from minigpt4_cpp_amd import modelgen as G, serve as S
    lib = gpu_lib
    vp, lp = os.path.join(tmpdir_models, "vision_guide.bin"), os.path.join(tmpdir_models, "llm_guide.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=31, std=0.05)
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=4096, n_layer=1, n_head=32, n_vocab=512, output_type="q6_k"), seed=4, std=0.02)
    reqs = [S.Request(G.synth_image(3 + i), p, n) for i, (p, n) in enumerate([("what is the text in the picture?", 6), ("describe it", 4), ("colour?", 5)])]
    srv, twin = (S.ReplicaServer(vp, lp, conversations=4, n_ctx=512, n_batch=64, library=lib) for _ in range(2))
    try:
        plain = twin.run(reqs, temp=0.0, ignore_eos=True)
        assert srv.run(reqs, temp=0.0, ignore_eos=True, guidance_scale=1.0) == plain          # 1.0 is today's loop ...
        assert lib.amd_guidance_info(srv.ctx)["launches"] == 0                                  # ... and touches none of this
        got = srv.run(reqs, temp=0.0, ignore_eos=True, guidance_scale=1.5)                      # three requests, two per wave: two waves
        assert got == _manual(lib, twin.ctx, reqs, 1.5, False, None, 4) and all(len(a) > 0 for a in got)
        launches = lib.amd_guidance_info(srv.ctx)["launches"]
        assert launches == 6 + 5                                                                # wave 1: max(6, 4) steps, wave 2: 5
        got_b = srv.run(reqs, temp=0.0, ignore_eos=True, guidance_scale=1.5, batched_prefill=True)
        assert got_b == _manual(lib, twin.ctx, reqs, 1.5, True, None, 4)
        neg = "a blurry photo of nothing"
        got_n = srv.run(reqs, temp=0.0, ignore_eos=True, guidance_scale=1.5, negative_prompt=neg)
        assert got_n == _manual(lib, twin.ctx, reqs, 1.5, False, neg, 4)
        print("plain", plain, "guided", got, "negative prompt", got_n)
        assert got_n != got or got != plain                                                     # the guidance conversation is what decides the difference
        stopped = srv.run(reqs, temp=0.0, guidance_scale=1.5)                                   # the decode loop's stop rule
        for x, y in zip(stopped, got):
            assert "###" not in x and len(x) <= len(y)
        with pytest.raises(ValueError):
            srv.run(reqs, guidance_scale=1.5, logprobs=1)
        with pytest.raises(ValueError):
            srv.run(reqs, guidance_scale=1.5, num_beams=2)
    finally:
        srv.close()
        twin.close()
