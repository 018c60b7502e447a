"""Sampled batched decode steps decided on the device: k_sample_rows alone against NumPy (tests/sampling_ref.py: Philox restated, the transformed row in fp32, the order by
lexsort, the rule in float64), then minigpt4_amd_sampled_candidates / _end_chat_batch_sampled / _conversation_seed on tiny model files against the same rule driven through
public calls, then the server.

Exact: candidate ids and n_cand, the Philox word, the stuck flag, the row tokens.  p_j: within 2e-4 relative of float64 -- for these inputs |w| <= 64, so the argument of
expf is off by at most about 1.6e-5, the 64-term sums add at most 4e-6, expf itself a few ulp: about 4e-5, and 2e-4 leaves a factor of five.  kept and the pick against the
float64 rule with two exclusions that the float64 reference alone decides: a row leaves the kept comparison when a reference cumulative sum lies within 1e-4 of top_p (its
kept may then differ by one, and the float64 rule is continued from the kernel's kept); a draw leaves the pick comparison when u lies within 1e-4 of a reference cumulative
boundary (the pick must still be one of the two neighbours).  Caps on the random rows: 5 % of a case's rows, 1 % of its draws (if a seed ever exceeds one: change the seed,
not the cap).  The constructed rows carry no cap: an all-equal row sits on the cut by construction (q_j = 1 / 40, and 36 / 40 is 0.9), which is the case the exclusion is for."""
import math
import os

import numpy as np
import pytest

import constraint_ref as R
import sampling_ref as SR
from test_cpu_penalties import penalise_ref

pytestmark = pytest.mark.gpu

PARAMS = [(0.8, 40, 0.9), (0.25, 64, 0.5), (1.5, 5, 1.0), (1.0, 1, 0.9)]
SHAPES = [(1, 100, 100), (3, 512, 512), (5, 513, 520), (2, 64, 72), (65, 32001, 32001)]
N_DRAWS = 32
PAD = np.float32(1e30)                                                       # the stride padding: it would win if it were read
REL, MARGIN = 2e-4, 1e-4


def f32_word(v):
    return int(np.array([v], np.float32).view(np.int32)[0])


def spec(row, table=(), pen=None, bitmap=None):
    """one logits row as a conversation presents it: table = [(id, count, bias, has_bias)], pen = SR.pen_row(...), bitmap = allowed words or None"""
    return dict(row=row, table=list(table), pen=pen or SR.pen_row(), bitmap=bitmap)


def run_and_check(lib, buf, V, specs, params, n_draws=N_DRAWS, what=""):
    """Every spec under n_draws draw counters in ONE launch, against the reference.  Returns (rows near the top_p cut, draws near a boundary, rows, draws)."""
    temp, top_k, top_p = params
    top_k = min(top_k, V)
    rows, table, bitmaps, bm_of, seed_draws = [], [], [], [], []
    for s_i, sp in enumerate(specs):
        off = len(table)
        table += [(t, c, f32_word(b), hb) for t, c, b, hb in sp["table"]]
        if sp["bitmap"] is not None:
            bitmaps.append(sp["bitmap"])
        pen = sp["pen"]
        seed = (1000 + 7 * s_i) | (s_i << 32)
        for c in range(n_draws):
            rows.append((sp["row"], off, len(sp["table"]), pen["flags"], f32_word(pen["repeat_penalty"]), f32_word(pen["alpha_frequency"]), f32_word(pen["alpha_presence"]), 0))
            bm_of.append(len(bitmaps) - 1 if sp["bitmap"] is not None else -1)
            seed_draws.append((seed, c * 0x9E37 + (1 << 40 if c % 4 == 3 else 0)))
    n = len(rows)
    tok = np.array([d if d < 48 else -1 for d in range(n)], np.int32)          # the first 48 descriptors hand their pick over, each to an entry of its own
    got = lib.amd_test_sample_rows(buf, V, np.array(rows, np.int32), np.array(table, np.int64).astype(np.int32).reshape(-1, 4), [(temp, top_p)] * n, [top_k] * n,
                                   np.array(seed_draws, np.uint64), bitmaps=np.array(bitmaps, np.uint32) if bitmaps else None, bitmap_of_row=bm_of, tok_index=tok)
    sd = np.array(seed_draws, np.uint64)
    words = SR.philox4x32_10(np.stack([sd[:, 1] & 0xFFFFFFFF, sd[:, 1] >> np.uint64(32), 0 * sd[:, 1], 0 * sd[:, 1]], -1), np.stack([sd[:, 0] & 0xFFFFFFFF, sd[:, 0] >> np.uint64(32)], -1))[:, 0]
    assert np.array_equal(got["word"], words), what                          # exact: the generator
    near_cut = near_edge = 0
    worst = 0.0
    for s_i, sp in enumerate(specs):
        trow = SR.transformed(buf[sp["row"], :V], sp["table"], sp["pen"])
        ids, vals = SR.candidates(trow, top_k, None if sp["bitmap"] is None else SR.bitmap_ids(sp["bitmap"], V))
        n_c = len(ids)
        excluded = None
        for c in range(n_draws):
            d = s_i * n_draws + c
            tag = f"{what} spec {s_i} draw {c}"
            assert got["n_cand"][d] == n_c, tag                                # exact: the selection
            assert np.array_equal(got["ids"][d][:n_c], ids) and (got["ids"][d][n_c:] == -1).all(), (tag, got["ids"][d][:n_c], ids)
            if n_c == 0:                                                       # nothing takes part: "</s>", flagged
                assert got["stuck"][d] == 1 and got["pick"][d] == SR.EOS and got["kept"][d] == 0 and (got["p"][d] == 0).all(), tag
                continue
            assert got["stuck"][d] == 0, tag
            ref = SR.rule64(vals, temp, top_p, int(words[d]))
            if excluded is None:
                excluded = ref["c"] is not None and float(np.abs(ref["c"] - float(np.float32(top_p))).min()) < MARGIN
                near_cut += excluded
            kept = int(got["kept"][d])
            if not excluded:
                assert kept == ref["kept"], (tag, kept, ref["kept"])
            else:
                assert abs(kept - ref["kept"]) <= 1 and 1 <= kept <= n_c, (tag, kept, ref["kept"])
                ref = SR.rule64(vals, temp, top_p, int(words[d]), kept=kept)
            p = got["p"][d].astype(np.float64)
            err = np.abs(p[:kept] - ref["p"])
            assert np.all(err <= REL * ref["p"]) and np.all(p[kept:] == 0), (tag, float(err.max()))
            nz = ref["p"] > 0
            worst = max(worst, float((err[nz] / ref["p"][nz]).max()))
            j = int(np.nonzero(ids == got["pick"][d])[0][0])                   # the pick is a candidate ...
            assert j < kept, tag                                               # ... that top-p kept
            if float(np.abs(ref["cum"] - ref["u"]).min()) >= MARGIN:
                assert j == ref["pick"], (tag, j, ref["pick"])
            else:
                near_edge += 1
                assert abs(j - ref["pick"]) <= 1, (tag, j, ref["pick"])
    for d in range(n):                                                         # the hand-over: written where an index was given, nowhere else
        if tok[d] >= 0:
            assert got["row_tok"][tok[d]] == got["pick"][d], (what, d)
    assert (got["row_tok"][min(n, 48):] == -7).all(), what
    n_rows, n_all = len(specs), n
    print(f"{what} temp {temp} top_k {top_k} top_p {top_p}: {n_rows} rows x {n_draws} draws, worst relative error of p {worst:.3g}, {near_cut} rows near the cut, "
          f"{near_edge} draws near a boundary, launch {got['ms'] * 1e3:.0f} us")
    return near_cut, near_edge, n_rows, n_all


def random_specs(rng, buf, V):
    """row r: r % 3 == 0 plain; 1: a penalty table that holds the row's first maximum (pushed down) and a biased id (pushed up); 2: the same under a random allowed set"""
    specs = []
    for r in range(len(buf)):
        if r % 3 == 0:
            specs.append(spec(r))
            continue
        top = int(np.argmax(buf[r, :V]))
        others = [int(i) for i in rng.permutation(V) if i != top][:13]
        table = [(top, 2, 0.0, 0)] + [(i, 1 + k % 3, 0.0, 0) for k, i in enumerate(others[:8])] + [(others[8], 1, 1.5, 1), (others[9], 0, 6.0, 1)] + \
                [(i, 0, float(b), 1) for i, b in zip(others[10:], (-2.0, 0.75, -0.5))]
        table.sort()                                                           # (any order will do; the engine's builder sorts the window ids)
        bitmap = SR.make_bitmap(V, [int(i) for i in np.nonzero(rng.random(V) < 0.5)[0]] + [top]) if r % 3 == 2 else None
        specs.append(spec(r, table, SR.pen_row(SR.PEN_REP | SR.PEN_ALPHA, 1.3, 0.25, 0.5), bitmap))
    return specs


@pytest.mark.parametrize("k,shape", list(enumerate(SHAPES)), ids=lambda v: "r%d_v%d_ld%d" % v if isinstance(v, tuple) else None)
def test_kernel_against_numpy(gpu_lib, k, shape):
    rows, V, ld = shape
    rng = np.random.default_rng(300 + k)
    buf = np.full((rows, ld), PAD, np.float32)
    buf[:, :V] = 3.0 * rng.standard_normal((rows, V)).astype(np.float32)
    specs = random_specs(rng, buf, V)
    cut = edge = n_rows = n_draws = 0
    for params in PARAMS:
        a, b, c, d = run_and_check(gpu_lib, buf, V, specs, params, what=f"shape {shape}")
        cut, edge, n_rows, n_draws = cut + a, edge + b, n_rows + c, n_draws + d
    assert cut <= 0.05 * n_rows and edge <= 0.01 * n_draws, (cut, n_rows, edge, n_draws)


def constructed(V, ld, rng):
    """(buf, specs): the rows the selection can go wrong on"""
    rows = []
    def add(row, **kw):
        rows.append((np.asarray(row, np.float32), kw))
    base = lambda: (3.0 * rng.standard_normal(V)).astype(np.float32)
    x = np.full(V, -5.0, np.float32); x[[7, V // 2, V - 2]] = (9.0, 8.0, 7.0); x[rng.permutation(V)[:300]] = 2.0   # ties across every top-k cut, more than 192 of them
    add(x)
    x = np.minimum(base(), 1.5); x[rng.permutation(V)[:10]] = 2.0                # ties across the cut that fit the tie list
    add(x)
    x = np.full(V, -1.0, np.float32); z = rng.permutation(V)[:12]; x[z] = np.where(np.arange(12) % 2 == 0, 0.0, -0.0)   # -0 and +0 tie: the order among them is by id
    add(x)
    add(np.full(V, 0.5, np.float32))                                             # an all-equal row
    x = base(); x[[0, 1, 2]] = (20.0, 19.0, 21.0); x[[V - 1, V - 2, V - 3]] = (20.5, 19.5, 18.5)   # winners in the scalar head and tail (ld is odd: every alignment occurs)
    add(x)
    x = base(); order = np.argsort(-x)                                           # a table that pushes the top id out of every cut and the 100th id in
    add(x, table=[(int(order[0]), 3, -30.0, 1), (int(order[min(99, V - 1)]), 0, 40.0, 1)], pen=SR.pen_row(SR.PEN_REP | SR.PEN_ALPHA, 1.3, 0.25, 0.5))
    x = base(); order = np.argsort(-x)                                           # a -infinity bias on the top id: it sorts last and is never drawn
    add(x, table=[(int(order[0]), 0, -math.inf, 1)])
    few = [int(i) for i in order[[0, 3, 50]]]                                    # an allowed set smaller than top_k, one of its ids at -infinity: it is a candidate with p = 0
    add(x, table=[(few[1], 0, -math.inf, 1)], bitmap=SR.make_bitmap(V, few))
    add(base(), bitmap=SR.make_bitmap(V, []))                                    # an empty allowed set
    x = np.full(V, 0.5, np.float32)                                              # all equal under a table: entries that stay in the tie (bias 0), one that leaves it, ids barred
    add(x, table=[(1, 0, 0.0, 1), (4, 0, 0.0, 1), (2, 1, 0.0, 0), (V - 1, 0, 0.0, 1)], pen=SR.pen_row(SR.PEN_REP, 1.3), bitmap=SR.make_bitmap(V, [i for i in range(V) if i not in (0, 3)]))
    buf = np.full((len(rows), ld), PAD, np.float32)
    for r, (x, _) in enumerate(rows):
        buf[r, :V] = x
    return buf, [spec(r, **kw) for r, (_, kw) in enumerate(rows)]


@pytest.mark.parametrize("V,ld,n_draws", [(513, 521, N_DRAWS), (32001, 32001, 8), (100, 101, N_DRAWS)], ids=lambda v: str(v))
def test_kernel_on_constructed_rows(gpu_lib, V, ld, n_draws):
    buf, specs = constructed(V, ld, np.random.default_rng(V))
    for params in PARAMS:
        run_and_check(gpu_lib, buf, V, specs, params, n_draws=n_draws, what=f"constructed V {V}")


# ------------------------------------------------------------------------------------------------ the engine
N_CTX = 96
PROMPT = "what is in the picture?"
PEN = dict(repeat_last_n=64, repeat_penalty=1.3, alpha_presence=0.0, alpha_frequency=0.0, penalize_nl=1)
BIAS = {90: -50.0, 41: 8.0, 51: 3.0}
PATTERN = r"[0-9]+"
PIECES = None


def pieces():
    global PIECES
    if PIECES is None:
        from minigpt4_cpp_amd import modelgen as G
        PIECES = [p for p, _ in G.synth_vocab(512)]                            # the tiny files' vocabulary
    return PIECES


def _load(lib, tiny_files, n_conv, seed=1337, n_ctx=N_CTX, conditioned=True):
    vp, llm = tiny_files
    ctx = lib.minigpt4_model_load(vp, llm("q5_k", mix="q5_k_m", conditioned=conditioned), verbosity=0, seed=seed, n_ctx=n_ctx, n_batch=32)
    lib.amd_set_conversations(ctx, n_conv)
    return ctx


def _n_past(lib, ctx, slot):
    lib.amd_select_conversation(ctx, slot)
    return int(lib.library.minigpt4_amd_n_past(ctx.ptr))


def _row(lib, ctx, slot):
    lib.amd_select_conversation(ctx, slot)
    return lib.amd_logits(ctx).copy()


def _hist(lib, ctx, slot):
    lib.amd_select_conversation(ctx, slot)
    return lib.amd_token_history(ctx).tolist()


def _setup(lib, ctx, handle=0, full_slot=None):
    """slot 0 plain, 1 a bias and repeat_penalty 1.3, 2 under the pattern (handle given), 3 plain -- or filled to the last row"""
    lib.amd_set_penalties(ctx, True)
    for s in range(4):
        lib.amd_select_conversation(ctx, s)
        lib.minigpt4_begin_chat(ctx, PROMPT + " " * s)
    lib.amd_select_conversation(ctx, 1)
    lib.amd_conversation_penalties(ctx, 1, **PEN)
    lib.amd_set_logit_bias(ctx, BIAS)
    if handle:
        lib.amd_set_constraint(ctx, 2, handle)
    if full_slot is not None:
        lib.amd_select_conversation(ctx, full_slot)
        lib.amd_logits(ctx)                                                    # the queue is evaluated
        n = N_CTX - _n_past(lib, ctx, full_slot)
        lib.amd_select_conversation(ctx, full_slot)
        lib.amd_eval_tokens(ctx, [5 + (7 * i) % 200 for i in range(n)])
        assert _n_past(lib, ctx, full_slot) == N_CTX
    lib.amd_select_conversation(ctx, 0)


def _reference(lib, ctx, slot, params, handle=0, state=0):
    """(candidate ids, values) of the rule on the conversation's raw row as public calls show it"""
    temp, top_k, top_p = params
    row = _row(lib, ctx, slot)
    if slot == 1:
        row = penalise_ref(row, _hist(lib, ctx, slot), N_CTX, bias=BIAS, **PEN)
    allowed = R.allowed_ids(lib.amd_constraint_mask(ctx, handle, state), len(row)) if handle and slot == 2 else None
    return SR.candidates(row, top_k, allowed)


def _check_pick(ids, vals, params, seed, draws, got_id, what):
    temp, top_k, top_p = params
    ref = SR.rule64(vals, temp, top_p, SR.draw_word(seed, draws))
    j = int(np.nonzero(ids == got_id)[0][0])
    near_cut = ref["c"] is not None and float(np.abs(ref["c"] - float(np.float32(top_p))).min()) < MARGIN
    if near_cut or float(np.abs(ref["cum"] - ref["u"]).min()) < MARGIN:
        assert abs(j - ref["pick"]) <= 1, what
    else:
        assert j == ref["pick"], (what, j, ref["pick"])


def test_sampled_candidates_equal_the_rule_and_move_nothing(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _load(lib, tiny_files, 4)
    try:
        h = lib.amd_constraint_compile(ctx, PATTERN)
        _setup(lib, ctx, h)
        slots = [2, 0, 1]
        for params in PARAMS:
            state = lib.amd_constraint_info(ctx, 2)["state"]
            before = [(_n_past(lib, ctx, s), _row(lib, ctx, s), _hist(lib, ctx, s), lib.amd_sampling_info(ctx, s)["draws"]) for s in slots]
            got = lib.amd_sampled_candidates(ctx, slots, *params)
            for i, s in enumerate(slots):
                ids, vals = _reference(lib, ctx, s, params, h, state)
                n_c = len(ids)
                assert got["n_cand"][i] == n_c == min(params[1], n_c) and np.array_equal(got["ids"][i][:n_c], ids) and (got["ids"][i][n_c:] == -1).all(), (params, s)
                ref = SR.rule64(vals, params[0], params[2], 0)
                near = ref["c"] is not None and float(np.abs(ref["c"] - float(np.float32(params[2]))).min()) < MARGIN
                kept = int(got["kept"][i])
                assert kept == ref["kept"] or (near and abs(kept - ref["kept"]) <= 1), (params, s)
                ref = SR.rule64(vals, params[0], params[2], 0, kept=kept)
                p = got["probs"][i].astype(np.float64)
                assert np.all(np.abs(p[:kept] - ref["p"]) <= REL * ref["p"]) and np.all(p[kept:] == 0), (params, s)
            after = [(_n_past(lib, ctx, s), _row(lib, ctx, s), _hist(lib, ctx, s), lib.amd_sampling_info(ctx, s)["draws"]) for s in slots]
            for a, b in zip(before, after):
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] == 0
            assert lib.amd_constraint_info(ctx, 2)["state"] == state
        assert len(_reference(lib, ctx, 2, PARAMS[0], h, state)[0]) < 40      # the pattern's start state allows fewer ids than top_k: the allowed set decides n_cand
        info = lib.amd_sampling_info(ctx, 0)
        assert info["launches"] == len(PARAMS) and info["handed"] == 0 and info["rows"] == 0
    finally:
        lib.minigpt4_free(ctx)


def test_sampled_step_equals_the_rule_and_a_forced_twin(gpu_lib, tiny_files):
    lib = gpu_lib
    a, b = _load(lib, tiny_files, 4), _load(lib, tiny_files, 4)
    params = PARAMS[0]
    slots = [1, 3, 0, 2]
    try:
        h = lib.amd_constraint_compile(a, PATTERN)
        trans = R.compile_ref(PATTERN.encode())[0]
        _setup(lib, a, h, full_slot=3)
        _setup(lib, b, 0, full_slot=3)
        state = lib.amd_constraint_info(a, 2)["state"]
        for step in range(6):
            refs = [_reference(lib, a, s, params, h, state) for s in slots]
            info0, pen0, con0 = lib.amd_sampling_info(a, 0), lib.amd_penalty_info(a), lib.amd_constraint_info(a, 2)
            past0 = [_n_past(lib, a, s) for s in slots]
            pcs, ids = lib.amd_end_chat_batch_sampled(a, slots, *params, with_ids=True)
            for i, s in enumerate(slots):
                seed = 1337 | (s << 32)                                        # the load seed and the slot
                assert lib.amd_sampling_info(a, s)["seed"] == seed and lib.amd_sampling_info(a, s)["draws"] == step + 1   # one draw each, the full one included
                _check_pick(refs[i][0], refs[i][1], params, seed, step, int(ids[i]), (step, s))
                assert pcs[i] == lib.amd_token_piece(a, int(ids[i]))
            twin = lib.amd_eval_batch(b, slots, [int(t) for t in ids])
            assert len(twin) == 4
            for i, s in enumerate(slots):
                assert _n_past(lib, a, s) == _n_past(lib, b, s) == past0[i] + (0 if s == 3 else 1), (step, s)
                assert np.array_equal(_row(lib, a, s), _row(lib, b, s)), (step, s)
                assert _hist(lib, a, s) == _hist(lib, b, s), (step, s)
            tid = int(ids[slots.index(2)])
            state = state if tid == R.EOS else R.walk(trans, state, pieces()[tid])
            assert lib.amd_constraint_info(a, 2)["state"] == state != R.DEAD   # the constraint state follows the pick
            info1, pen1, con1 = lib.amd_sampling_info(a, 0), lib.amd_penalty_info(a), lib.amd_constraint_info(a, 2)
            assert info1["launches"] == info0["launches"] + 1 and info1["handed"] == info0["handed"] + 3 and info1["rows"] == info0["rows"] + 4
            assert pen1["host_rows"] == pen0["host_rows"] and pen1["launches"] == pen0["launches"]      # no row went to the host chain, no other pick kernel ran
            assert con1["host_rows"] == con0["host_rows"] and con1["pick_launches"] == con0["pick_launches"]
        assert _n_past(lib, a, 3) == N_CTX
        assert lib.amd_sampling_info(b, 0)["launches"] == 0                    # the twin never launched the kernel
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


def _run8(lib, ctx, slots, n=8, params=PARAMS[2]):
    out = []
    for _ in range(n):
        out.append(lib.amd_end_chat_batch_sampled(ctx, slots, *params, with_ids=True)[1].copy())
    return np.array(out)


def _prompt(lib, ctx, slot, text):
    lib.amd_select_conversation(ctx, slot)
    lib.minigpt4_reset_chat(ctx)
    lib.minigpt4_begin_chat(ctx, text)


def test_a_seeded_conversation_does_not_depend_on_its_company(gpu_lib, tiny_files):
    lib = gpu_lib
    a, b = _load(lib, tiny_files, 4, n_ctx=256, conditioned=False), _load(lib, tiny_files, 4, seed=99, n_ctx=256, conditioned=False)
    try:
        for c in (a, b):
            lib.amd_set_parity(c, True)
        runs = []
        for c, slot, listing in ((a, 0, [0]), (a, 0, [0, 1, 2, 3]), (a, 0, [3, 2, 0, 1]), (a, 2, [1, 2]), (b, 1, [0, 1, 3])):   # alone, with partners, elsewhere in the list, another slot, another context
            for s in listing:
                _prompt(lib, c, s, PROMPT if s == slot else f"partner {s} of {len(listing)}")
                lib.amd_conversation_seed(c, s, 4242 if s == slot else 17 + s, 0)
            runs.append(_run8(lib, c, listing)[:, listing.index(slot)])
            assert lib.amd_sampling_info(c, slot)["draws"] == 8
        for r in runs[1:]:
            assert np.array_equal(r, runs[0]), (runs[0], r)
        assert len(set(runs[0].tolist())) > 1                                  # (a run of one repeated token would show little)
        # another seed gives another text; draws = k continues the stream: the first five fed by hand, the rest sampled from draw 5 on
        others = []
        for seed in (4243, 1 << 40, (1 << 64) - 1):
            _prompt(lib, a, 0, PROMPT)
            lib.amd_conversation_seed(a, 0, seed, 0)
            others.append(_run8(lib, a, [0])[:, 0])
        assert any(not np.array_equal(o, runs[0]) for o in others)
        _prompt(lib, a, 0, PROMPT)
        lib.amd_select_conversation(a, 0)
        lib.amd_eval_tokens(a, [int(t) for t in runs[0][:5]])
        lib.amd_conversation_seed(a, 0, 4242, 5)
        assert np.array_equal(_run8(lib, a, [0], n=3)[:, 0], runs[0][5:])
        assert lib.amd_sampling_info(a, 0)["draws"] == 8
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


def test_refusals_leave_everything_untouched(gpu_lib, tiny_files):
    import ctypes
    lib = gpu_lib
    ctx = _load(lib, tiny_files, 4)
    I32P = ctypes.POINTER(ctypes.c_int32)
    try:
        for s in (0, 1):
            _prompt(lib, ctx, s, PROMPT)
        lib.amd_conversation_seed(ctx, 0, 5, 3)
        L = lib.library
        toks, ids = (ctypes.c_char_p * 4)(), np.zeros(4 * 64, np.int32)

        def snapshot():
            return [(_n_past(lib, ctx, s), lib.amd_sampling_info(ctx, s)) for s in range(4)], _hist(lib, ctx, 0)

        def step(slots, temp=0.8, top_k=40, top_p=0.9, tokens=toks):
            sl = np.array(slots, np.int32)
            return L.minigpt4_amd_end_chat_batch_sampled(ctx.ptr, sl.ctypes.data_as(I32P) if len(sl) else None, len(sl), tokens, temp, top_k, top_p, ids.ctypes.data_as(I32P))

        def cand(slots, temp=0.8, top_k=40, top_p=0.9):
            sl = np.array(slots, np.int32)
            return L.minigpt4_amd_sampled_candidates(ctx.ptr, sl.ctypes.data_as(I32P) if len(sl) else None, len(sl), temp, top_k, top_p, ids.ctypes.data_as(I32P), None, None, None)
        lib.amd_select_conversation(ctx, 0)
        lib.amd_logits(ctx)
        before = snapshot()
        for f, name in ((step, b"end_chat_batch_sampled: "), (cand, b"sampled_candidates: ")):
            for args, kw in ((([],), {}), (([0, 0],), {}), (([0, 4],), {}), (([0, -1],), {}), (([0, 1, 2, 3, 0],), {}),
                             (([0],), dict(temp=0.0)), (([0],), dict(temp=-0.5)), (([0],), dict(temp=float("nan"))), (([0],), dict(temp=float("inf"))),
                             (([0],), dict(top_k=0)), (([0],), dict(top_k=65)), (([0],), dict(top_k=-3)),
                             (([0],), dict(top_p=0.0)), (([0],), dict(top_p=1.0001)), (([0],), dict(top_p=float("nan"))),
                             (([0, 2],), {})):                                 # conversation 2 has nothing queued and nothing evaluated
                assert f(*args, **kw) == 1, (name, args, kw)
                assert L.minigpt4_amd_last_error().startswith(name), L.minigpt4_amd_last_error()
            assert b"conversation 2 has no current logits" in L.minigpt4_amd_last_error()
        assert step([0], tokens=None) == 1 and L.minigpt4_amd_last_error().startswith(b"end_chat_batch_sampled: tokens")
        assert L.minigpt4_amd_conversation_seed(ctx.ptr, 4, 1, 1) == 1 and L.minigpt4_amd_last_error().startswith(b"conversation_seed: ")
        assert L.minigpt4_amd_sampling_info(ctx.ptr, -1, np.zeros(6, np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == 1
        assert L.minigpt4_amd_sampling_info(ctx.ptr, 0, None) == 1 and L.minigpt4_amd_last_error().startswith(b"sampling_info: ")
        lib.amd_select_conversation(ctx, 0)
        assert snapshot() == before
        assert before[0][0][1]["seed"] == 5 and before[0][0][1]["draws"] == 3 and before[0][0][1]["launches"] == 0   # nothing was launched, nothing allocated
        # n_vocab = 512 >= 64: top_k = 64 is accepted, ids_out may be NULL
        sl = np.array([0, 1], np.int32)
        assert L.minigpt4_amd_end_chat_batch_sampled(ctx.ptr, sl.ctypes.data_as(I32P), 2, toks, 0.8, 64, 1.0, None) == 0
        assert lib.amd_sampling_info(ctx, 0)["draws"] == 4 and lib.amd_sampling_info(ctx, 1)["draws"] == 1
        # reset_chat and set_conversations: the first keeps the pair, the second returns it to the load seed
        lib.amd_select_conversation(ctx, 0)
        lib.minigpt4_reset_chat(ctx)
        assert lib.amd_sampling_info(ctx, 0)["seed"] == 5 and lib.amd_sampling_info(ctx, 0)["draws"] == 4
        lib.amd_set_conversations(ctx, 2)
        i1 = lib.amd_sampling_info(ctx, 1)
        assert i1["seed"] == 1337 | (1 << 32) and i1["draws"] == 0
    finally:
        lib.minigpt4_free(ctx)


def test_the_host_chain_is_what_it_was(gpu_lib, tiny_files):
    """end_chat_batch at temp 0.8 draws from the context's mt19937: the same ids whether or not other conversations of the context use the device path in between"""
    lib = gpu_lib
    a, b = _load(lib, tiny_files, 4, n_ctx=256), _load(lib, tiny_files, 4, n_ctx=256)
    try:
        for c in (a, b):
            for s in range(4):
                _prompt(lib, c, s, PROMPT + " " * s)
        got = {a: [], b: []}
        for step in range(5):
            lib.amd_end_chat_batch_sampled(a, [2, 3], *PARAMS[0])
            for c in (a, b):
                got[c].append(lib.amd_end_chat_batch(c, [0, 1], temp=0.8, top_k=40, top_p=0.9))
        assert got[a] == got[b]
        for s in (0, 1):
            assert _hist(lib, a, s) == _hist(lib, b, s)
            assert lib.amd_sampling_info(a, s)["draws"] == 0                   # the host chain counts no draw of the conversation's stream
        assert lib.amd_sampling_info(a, 2)["draws"] == 5 and lib.amd_sampling_info(b, 0)["launches"] == 0
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


def test_server_device_sampling_keyword(gpu_lib, tmpdir_models):
    from minigpt4_cpp_amd import modelgen as G, serve as S
    vp, lp = os.path.join(tmpdir_models, "vision_serve_smp.bin"), os.path.join(tmpdir_models, "llm_serve_smp.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=31, std=0.05)                       # tests/test_gpu_serve.py's model
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=4096, n_layer=1, n_head=32, n_vocab=512, output_type="q6_k"), seed=4, std=0.02)
    reqs = [S.Request(G.synth_image(3 + i), p, 10) for i, p in enumerate(["what is the text in the picture?", "describe it", "colour?"])]
    seeds = [11, 22, 33]
    srv = S.ReplicaServer(vp, lp, conversations=2, n_ctx=512, n_batch=64, library=gpu_lib)           # waves of 2 + 1
    try:
        srv.lib.amd_set_parity(srv.ctx, True)                                  # logits that do not depend on the batch: the text depends on the seed alone
        kw = dict(temp=0.8, top_k=40, top_p=0.9, ignore_eos=True, device_sampling=True)
        together = srv.run(reqs, seeds=seeds, **kw)
        assert srv.run([reqs[1]], seeds=[seeds[1]], **kw) == [together[1]]       # alone, in slot 0 instead of slot 1
        assert srv.run(reqs[::-1], seeds=seeds[::-1], **kw) == together[::-1]    # other partners, other slots
        assert len(set(together)) == 3 and all(together)
        info = srv.lib.amd_sampling_info(srv.ctx, 0)
        assert info["launches"] > 0 and info["rows"] >= 30
        extra = dict(regex=r"[a-z]+ [0-9]+", repeat_penalty=1.3, logit_bias={41: 4.0})   # with a pattern, penalties and a bias
        x = srv.run(reqs, seeds=seeds, **{**kw, **extra})
        assert srv.run([reqs[1]], seeds=[seeds[1]], **{**kw, **extra}) == [x[1]]
        with pytest.raises(ValueError):
            srv.run(reqs, seeds=seeds, num_beams=2, **kw)
    finally:
        srv.close()
