"""Draft verification under sampling (minigpt4_amd_verify_draft_sampled / _decode_lookup_sampled / _speculation_info; kernels k_sample_rows + k_draft_sample_finish).

1. The epilogue alone (minigpt4_amd_test_draft_sample): the picks against the float64 rule of tests/sampling_ref.py with the exclusions and bounds of
   tests/test_gpu_device_sampling.py (candidate ids and the Philox word exact; REL = 2e-4 and MARGIN = 1e-4 as derived there; at most 5 % of a case's random rows near the
   top-p cut and 1 % of its draws near a boundary -- conditions on the seeds, counted by the float64 reference alone in a test that needs no GPU); m, the slot's logits row,
   its first argmax, the position and the other slot exactly.
2. Through the C ABI in fast mode: every evaluated row's sample equals the rule on the raw row the call reports, transformed with the history and the constraint state as
   of that row, under draw c + 1 + r; everything the call leaves behind follows from those samples and the draft; a twin advanced by minigpt4_amd_eval_batch over the kept ids
   agrees within the bound tests/test_gpu_draft.py holds a verify pass to against single rows (1e-2 of the largest |logit|, and 2 x the recorded error).
3. Parity mode: the lookup loop emits, token for token, what a plain minigpt4_amd_end_chat_batch_sampled loop emits from the same (seed, draws).
4. Refusals leave everything untouched; the greedy verify pass and its graphs are what they were."""
import ctypes

import numpy as np
import pytest

import constraint_ref as R
import sampling_ref as SR
from conftest import observed_bar
from test_cpu_penalties import penalise_ref
from test_gpu_device_sampling import BIAS, MARGIN, PAD, PARAMS, PATTERN, PEN, PROMPT, REL, _check_pick, _hist, _n_past, _row, constructed, f32_word, pieces, random_specs

gpu = pytest.mark.gpu
RS = [1, 2, 5, 8]
VLD = [(100, 101), (513, 520), (32001, 32001), (512, 512)]                    # (512, 512): the 16-byte loads of the copy sweep
COUNTERS = [0, 3 * 0x9E37 + (1 << 40)]                                        # the call's c: row r draws with c + 1 + r
CONSTRUCTED_ROWS = {1: [8], 2: [3, 8], 5: [0, 2, 3, 8, 9], 8: [0, 1, 2, 3, 4, 5, 8, 9]}   # 8: an empty allowed set, 3: all equal, 0 / 1: ties across the cut, 2: -0 / +0
SEED0 = 703                                                                    # 700 .. 702 put a row within 1e-4 of a top-p cut (if a case ever exceeds a cap: change this, not the cap)


def case_rows(R_, V, ld, source):
    """(buf [R][ld], specs with descriptor r on row r)"""
    rng = np.random.default_rng(SEED0 + 31 * R_ + V)
    if source == "random":
        buf = np.full((R_, ld), PAD, np.float32)
        buf[:, :V] = 3.0 * rng.standard_normal((R_, V)).astype(np.float32)
        if R_ > 1:
            buf[1, [5, V - 3]] = buf[1, :V].max() + np.float32(1.0)            # two equal maxima: the first one is the greedy token
            buf[R_ - 1, :V] = np.where(buf[R_ - 1, :V] > 6.0, 6.0, buf[R_ - 1, :V])
        return buf, random_specs(rng, buf, V)
    all_buf, all_specs = constructed(V, ld, rng)
    keep = CONSTRUCTED_ROWS[R_]
    buf = np.ascontiguousarray(all_buf[keep])
    return buf, [dict(all_specs[k], row=r) for r, k in enumerate(keep)]


def descriptors(specs, c, seed=4242 | (3 << 32)):
    rows, table, bitmaps, bm_of, sd = [], [], [], [], []
    for r, sp in enumerate(specs):
        off = len(table)
        table += [(t, n, f32_word(b), hb) for t, n, b, hb in sp["table"]]
        if sp["bitmap"] is not None:
            bitmaps.append(sp["bitmap"])
        pen = sp["pen"]
        rows.append((r, off, len(sp["table"]), pen["flags"], f32_word(pen["repeat_penalty"]), f32_word(pen["alpha_frequency"]), f32_word(pen["alpha_presence"]), 0))
        bm_of.append(len(bitmaps) - 1 if sp["bitmap"] is not None else -1)
        sd.append((seed, c + 1 + r))
    return dict(rows=np.array(rows, np.int32), table=np.array(table, np.int64).astype(np.int32).reshape(-1, 4), bitmaps=np.array(bitmaps, np.uint32) if bitmaps else None,
                bitmap_of_row=bm_of, seed_draws=np.array(sd, np.uint64))


def reference(buf, V, specs, params, seed_draws):
    """per row: None (nothing takes part) or (ids, vals, rule64 result, near the cut, near a boundary) -- float64, no GPU"""
    temp, top_k, top_p = params
    out = []
    for r, sp in enumerate(specs):
        trow = SR.transformed(buf[r, :V], sp["table"], sp["pen"])
        ids, vals = SR.candidates(trow, min(top_k, V), None if sp["bitmap"] is None else SR.bitmap_ids(sp["bitmap"], V))
        if len(ids) == 0:
            out.append(None)
            continue
        ref = SR.rule64(vals, temp, top_p, SR.draw_word(int(seed_draws[r][0]), int(seed_draws[r][1])))
        near_cut = ref["c"] is not None and float(np.abs(ref["c"] - float(np.float32(top_p))).min()) < MARGIN
        near_edge = float(np.abs(ref["cum"] - ref["u"]).min()) < MARGIN
        out.append((ids, vals, ref, near_cut, near_edge))
    return out


@pytest.mark.parametrize("V,ld", VLD, ids=lambda v: str(v))
@pytest.mark.parametrize("R_", RS)
def test_reference_exclusions_are_within_the_caps(R_, V, ld):
    """no GPU: the random rows of every case keep the exclusions within 5 % of the rows and 1 % of the draws (a condition on SEED0, decided by the float64 reference)"""
    buf, specs = case_rows(R_, V, ld, "random")
    cut = edge = n = 0
    for params in PARAMS:
        for c in COUNTERS:
            for ref in reference(buf, V, specs, params, descriptors(specs, c)["seed_draws"]):
                if ref is not None:
                    cut, edge, n = cut + ref[3], edge + ref[4], n + 1
    assert cut <= 0.05 * n and edge <= 0.01 * n, (cut, edge, n)


def check_picks(got, buf, V, specs, params, d, what):
    temp, top_k, top_p = params
    sd = d["seed_draws"]
    for r, ref in enumerate(reference(buf, V, specs, params, sd)):
        tag = (what, r)
        assert int(got["word"][r]) == SR.draw_word(int(sd[r][0]), int(sd[r][1])), tag      # exact: the generator
        if ref is None:
            assert got["stuck"][r] == 1 and got["pick"][r] == SR.EOS and got["n_cand"][r] == 0 and got["kept"][r] == 0, tag
            continue
        ids, vals, ref, near_cut, near_edge = ref
        n_c = len(ids)
        assert got["stuck"][r] == 0 and got["n_cand"][r] == n_c, tag
        assert np.array_equal(got["ids"][r][:n_c], ids) and (got["ids"][r][n_c:] == -1).all(), tag   # exact: the selection
        kept = int(got["kept"][r])
        if not near_cut:
            assert kept == ref["kept"], (tag, kept, ref["kept"])
        else:
            assert abs(kept - ref["kept"]) <= 1 and 1 <= kept <= n_c, (tag, kept, ref["kept"])
            ref = SR.rule64(vals, temp, top_p, int(got["word"][r]), kept=kept)
        p = got["p"][r].astype(np.float64)
        assert np.all(np.abs(p[:kept] - ref["p"]) <= REL * ref["p"]) and np.all(p[kept:] == 0), tag
        j = int(np.nonzero(ids == got["pick"][r])[0][0])
        assert j < kept, tag
        if float(np.abs(ref["cum"] - ref["u"]).min()) >= MARGIN:
            assert j == ref["pick"], (tag, j, ref["pick"])
        else:
            assert abs(j - ref["pick"]) <= 1, (tag, j, ref["pick"])


@gpu
@pytest.mark.parametrize("V,ld", VLD, ids=lambda v: str(v))
@pytest.mark.parametrize("R_", RS)
def test_epilogue_alone(gpu_lib, R_, V, ld):
    lib = gpu_lib
    rng = np.random.default_rng(R_ + V)
    for source in ("random", "constructed"):
        buf, specs = case_rows(R_, V, ld, source)
        for k, params in enumerate(PARAMS):
            c = COUNTERS[k % 2]
            d = descriptors(specs, c)
            state = np.array([[17, 400 % V, 401 % V], [90, 7, 8]], np.int32)
            keep = (0.25 * rng.standard_normal((2, V))).astype(np.float32)
            call = lambda tok, slot: lib.amd_test_draft_sample(buf, V, d["rows"], d["table"], [(params[0], params[2])] * R_, [min(params[1], V)] * R_, d["seed_draws"], tok, slot,
                                                               state, keep, bitmaps=d["bitmaps"], bitmap_of_row=d["bitmap_of_row"])
            first = call([-1] * R_, 0)                                          # no row token equals a pick: m = 0, and the picks are learnt
            what = (source, R_, V, params)
            check_picks(first, buf, V, specs, params, d, what)
            picks = first["pick"]
            assert first["m"] == 0 and np.array_equal(first["picks"], picks) and np.array_equal(first["stuck_flags"], first["stuck"]), what
            assert (first["res"][1 + R_:9] == -1).all() and (first["res"][9 + R_:] == -1).all(), what     # entries behind R are left alone
            for j in sorted({0, (R_ - 1) // 2, R_ - 1}):
                slot = (j + k) % 2
                tok = np.full(R_, -1, np.int32)
                tok[0] = 123 % V                                                 # x0: never compared
                tok[1:1 + j] = picks[:j]                                          # right up to j ...
                if j + 1 < R_:
                    tok[j + 1] = (picks[j] + 1) % V                               # ... wrong at j ...
                    tok[j + 2:] = picks[j + 1:R_ - 1]                             # ... and right again behind it: only the first mismatch counts
                got = call(tok, slot)
                tag = (what, j, slot)
                assert got["m"] == j, (tag, got["m"])
                assert np.array_equal(got["pick"], picks) and np.array_equal(got["picks"], picks) and np.array_equal(got["stuck_flags"], first["stuck"]), tag
                row = buf[j, :V]
                assert np.array_equal(got["slot_logits"][slot].view(np.uint32), row.view(np.uint32)), tag       # the row, bit for bit (the padding was not read)
                first_max = int(np.argmax(row))                                  # numpy: the first of equal maxima, -0.0 == +0.0
                assert got["state"][slot].tolist() == [state[slot][0] + 1 + j, first_max, first_max], (tag, got["state"][slot], first_max)
                other = 1 - slot
                assert got["state"][other].tolist() == state[other].tolist() and np.array_equal(got["slot_logits"][other].view(np.uint32), keep[other].view(np.uint32)), tag
        print(f"k_draft_sample_finish {source} R {R_} V {V} ld {ld}: {got['ms'] * 1e3:.0f} us")


# ------------------------------------------------------------------------------------------------ the engine
N_CTX = 256
SEED = 1337


def _load(lib, tiny_files, n_conv, parity=False, max_draft=7, n_ctx=N_CTX):
    vp, llm = tiny_files
    ctx = lib.minigpt4_model_load(vp, llm("q5_k", mix="q5_k_m", conditioned=True), verbosity=0, seed=SEED, n_ctx=n_ctx, n_batch=32)
    lib.amd_set_conversations(ctx, n_conv)
    if parity:
        lib.amd_set_parity(ctx, True)
    lib.amd_set_speculation(ctx, max_draft)
    return ctx


def _setup(lib, ctx, handle):
    """slot 0 plain, 1 a bias and repeat_penalty 1.3, 2 under the pattern (handle given), 3 plain"""
    lib.amd_set_penalties(ctx, True)
    for s in range(4):
        lib.amd_select_conversation(ctx, s)
        lib.minigpt4_begin_chat(ctx, PROMPT + " " * s)
    lib.amd_select_conversation(ctx, 1)
    lib.amd_conversation_penalties(ctx, 1, **PEN)
    lib.amd_set_logit_bias(ctx, BIAS)
    if handle:
        lib.amd_set_constraint(ctx, 2, handle)
    lib.amd_select_conversation(ctx, 0)


def _snapshot(lib, ctx, slot):
    info = lib.amd_sampling_info(ctx, slot)
    return dict(p=_n_past(lib, ctx, slot), row=_row(lib, ctx, slot), hist=_hist(lib, ctx, slot), draws=info["draws"], seed=info["seed"],
                state=lib.amd_constraint_info(ctx, slot)["state"], spec=lib.amd_speculation_info(ctx), smp=(info["launches"], info["rows"], info["handed"]))


def _same(a, b):
    return a["p"] == b["p"] and np.array_equal(a["row"], b["row"]) and a["hist"] == b["hist"] and a["draws"] == b["draws"] and a["seed"] == b["seed"] and \
        a["state"] == b["state"] and a["spec"] == b["spec"] and a["smp"] == b["smp"]


def _rule_candidates(lib, ctx, slot, raw, hist, handle, state, params):
    """(ids, values): the candidates of the rule on a raw row, transformed with `hist` (slot 1: its bias and penalty) under constraint state `state` (slot 2)"""
    row = penalise_ref(raw, hist, N_CTX, bias=BIAS, **PEN) if slot == 1 else np.asarray(raw, np.float32)
    allowed = R.allowed_ids(lib.amd_constraint_mask(ctx, handle, state), len(row)) if handle and slot == 2 else None
    return SR.candidates(row, params[1], allowed)


@gpu
def test_calls_follow_the_rule_and_leave_what_it_says(gpu_lib, tiny_files):
    lib = gpu_lib
    params = PARAMS[0]
    a, b, scout = _load(lib, tiny_files, 5), _load(lib, tiny_files, 4), _load(lib, tiny_files, 4)
    try:
        h = lib.amd_constraint_compile(a, PATTERN)
        hs = lib.amd_constraint_compile(scout, PATTERN)
        trans = R.compile_ref(PATTERN.encode())[0]
        _setup(lib, a, h)
        _setup(lib, b, 0)
        _setup(lib, scout, hs)
        assert lib.amd_speculation_info(a) == dict.fromkeys(lib.SPECULATION_INFO_FIELDS, 0)
        ahead = {s: [] for s in range(4)}            # what plain sampled decoding emits from the same state: the scout's recorded samples, the source of every draft
        emitted = {s: [] for s in range(4)}
        announced = {}
        kinds = set()
        bar = observed_bar("verify_draft_q5_k_q5_k_m")
        worst = 0.0
        for rnd in range(6):
            for n_draft in (0, 1, 3, 7):
                for s in range(4):
                    k = len(emitted[s])
                    while len(ahead[s]) < k + 1 + n_draft:
                        ahead[s].append(int(lib.amd_end_chat_batch_sampled(scout, [s], *params, with_ids=True)[1][0]))
                    draft = ahead[s][k + 1:k + 1 + n_draft]
                    kind = ("all", "first", "middle")[(rnd + s) % 3] if n_draft else "none"
                    wrong = {"first": 0, "middle": n_draft // 2}.get(kind)
                    if wrong is not None:
                        draft[wrong] = 3 + 0x30 + (draft[wrong] - 3 - 0x30 + 1) % 10 if s == 2 else (draft[wrong] + 1) % 512   # (slot 2: another digit, so that the constraint lets the row run)
                    before = _snapshot(lib, a, s)
                    lib.amd_select_conversation(a, s)
                    r = lib.amd_verify_draft_sampled(a, draft, *params, want_rows=True, want_logits=True)
                    after = _snapshot(lib, a, s)
                    tag = (rnd, n_draft, s, kind)
                    ids, rs = [int(t) for t in r["ids"]], r["row_sampled"]
                    seed, c = before["seed"], before["draws"]
                    assert seed == SEED | (s << 32)
                    # x0 = D(L, h, q, c)
                    cand = _rule_candidates(lib, a, s, before["row"], before["hist"], h, before["state"], params)
                    _check_pick(cand[0], cand[1], params, seed, c, ids[0], tag)
                    if s in announced:
                        assert ids[0] == announced[s], tag                       # what the call before announced
                    # the rows: history and state as of row r, draw c + 1 + r; the cut by the state's index row
                    toks = [ids[0]] + draft
                    state, hist, n_rows = before["state"], list(before["hist"]), 0
                    states = []
                    for i, t in enumerate(toks):
                        if i and s == 2 and t not in R.allowed_ids(lib.amd_constraint_mask(a, h, state), 512):
                            break
                        if s == 2 and t != R.EOS:
                            state = R.walk(trans, state, pieces()[t])
                        hist.append(t)
                        states.append(state)
                        n_rows += 1
                        assert rs[i] >= 0, (tag, i, rs)
                        cand = _rule_candidates(lib, a, s, r["row_logits"][i], hist, h, state, params)
                        _check_pick(cand[0], cand[1], params, seed, c + 1 + i, int(rs[i]), (tag, i))
                    assert (rs[n_rows:] == -1).all() and np.isnan(r["row_logits"][n_rows:]).all(), tag
                    assert n_rows == 1 + n_draft, tag                            # (these drafts hold nothing the pattern forbids)
                    m = 0
                    while m < n_rows - 1 and draft[m] == rs[m]:
                        m += 1
                    assert ids == toks[:1 + m] and r["next"] == rs[m], (tag, ids, toks, rs)
                    assert np.array_equal(lib.amd_logits(a), r["row_logits"][m]), tag
                    assert after["p"] == before["p"] + 1 + m and after["hist"] == before["hist"] + ids and after["draws"] == c + 1 + m, tag
                    assert after["state"] == (states[m] if s == 2 else 0) and after["smp"] == before["smp"], tag
                    sp0, sp1 = before["spec"], after["spec"]
                    assert (sp1["passes"], sp1["rows"], sp1["sent"], sp1["accepted"], sp1["launches"], sp1["cut"]) == \
                        (sp0["passes"] + 1, sp0["rows"] + n_rows, sp0["sent"] + n_rows - 1, sp0["accepted"] + m, sp0["launches"] + 2, sp0["cut"]), tag
                    announced[s] = r["next"]
                    emitted[s] += ids
                    if n_draft:
                        kinds.add("all" if m == n_draft else "first" if m == 0 else "middle")
                    # rejected rows never leak: the twin takes the kept ids one at a time
                    for t in ids:
                        lib.amd_eval_batch(b, [s], [t])
                    assert _n_past(lib, b, s) == after["p"] and _hist(lib, b, s) == after["hist"], tag
                    want = _row(lib, b, s)
                    err = float(np.abs(after["row"] - want).max() / np.abs(want).max())
                    worst = max(worst, err)
                    assert err <= bar, (tag, err, bar)
        print(f"verify_draft_sampled against a twin fed single rows: {worst:.3e} of the largest |logit| (bar {bar:.3e}); accepted {lib.amd_speculation_info(a)}")
        assert kinds == {"all", "first", "middle"}, kinds                        # all accepted, first wrong and middle wrong each occurred
        # a draft holding a letter under the pattern is cut and counted
        lib.amd_select_conversation(a, 2)
        letter = next(i for i, p in enumerate(pieces()) if i >= 3 and p.isalpha())
        sp0 = lib.amd_speculation_info(a)
        r = lib.amd_verify_draft_sampled(a, [3 + 0x31, letter, 3 + 0x32], *params, want_rows=True)
        sp1 = lib.amd_speculation_info(a)
        assert (r["row_sampled"][:2] >= 0).all() and (r["row_sampled"][2:] == -1).all() and sp1["cut"] == sp0["cut"] + 2 and sp1["rows"] == sp0["rows"] + 2 and \
            sp1["sent"] == sp0["sent"] + 1
        # n_draft = 0 picks what end_chat_batch_sampled picks for that slot from the same state: a forked twin with the stream copied
        lib.amd_fork_conversation(a, 0, [4])
        info = lib.amd_sampling_info(a, 0)
        lib.amd_conversation_seed(a, 4, info["seed"], info["draws"])
        lib.amd_select_conversation(a, 0)
        r = lib.amd_verify_draft_sampled(a, [], *params)
        assert int(r["ids"][0]) == announced[0]
        assert int(lib.amd_end_chat_batch_sampled(a, [4], *params, with_ids=True)[1][0]) == int(r["ids"][0])
        assert lib.amd_sampling_info(a, 4)["draws"] == lib.amd_sampling_info(a, 0)["draws"] == info["draws"] + 1
        assert np.array_equal(_row(lib, a, 0), _row(lib, a, 4))                  # one row through the verify pass is the batched step at one row
    finally:
        for c in (a, b, scout):
            lib.minigpt4_free(c)


@gpu
def test_parity_lookup_equals_the_plain_sampled_loop(gpu_lib, tiny_files):
    lib = gpu_lib
    params = PARAMS[0]
    ctx = _load(lib, tiny_files, 2, parity=True, max_draft=4)
    try:
        lib.minigpt4_begin_chat(ctx, PROMPT)
        lib.amd_conversation_seed(ctx, 0, 99, 5)
        lib.amd_fork_conversation(ctx, 0, [1])
        lib.amd_conversation_seed(ctx, 1, 99, 5)
        plain = [int(lib.amd_end_chat_batch_sampled(ctx, [1], *params, with_ids=True)[1][0]) for _ in range(24)]
        if R.EOS in plain:
            plain = plain[:plain.index(R.EOS) + 1]                               # the lookup loop ends behind "</s>"; the plain loop does not know it
        lib.amd_select_conversation(ctx, 0)
        r = lib.amd_decode_lookup_sampled(ctx, plain, 24, ngram_max=3, ngram_min=1, n_draft=4, temp=params[0], top_k=params[1], top_p=params[2])   # the corpus: the text itself
        got = [int(t) for t in r["tokens"]]
        assert got == plain, (got, plain)
        assert r["passes"] + r["steps"] + r["accepted"] == len(got)
        assert r["passes"] > 0 and r["accepted"] > 0 and r["sent"] >= r["accepted"], r      # the drafter fired and its drafts were kept
        assert lib.amd_sampling_info(ctx, 0)["draws"] == 5 + len(got)
        assert _n_past(lib, ctx, 0) == _n_past(lib, ctx, 1) - (24 - len(got)) and _hist(lib, ctx, 0) == _hist(lib, ctx, 1)[:len(_hist(lib, ctx, 0))]
        if len(got) == 24:
            assert np.array_equal(_row(lib, ctx, 0), _row(lib, ctx, 1))          # oracle-order passes: the same logits bit for bit
        info = lib.amd_speculation_info(ctx)
        assert info["accepted"] == r["accepted"] and info["sent"] == r["sent"] and info["passes"] == r["passes"] + r["steps"]
    finally:
        lib.minigpt4_free(ctx)


@gpu
def test_refusals_leave_everything_untouched(gpu_lib, tiny_files):
    lib = gpu_lib
    L = lib.library
    I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    ctx = _load(lib, tiny_files, 3, max_draft=0, n_ctx=96)
    try:
        h = lib.amd_constraint_compile(ctx, PATTERN)
        lib.minigpt4_begin_chat(ctx, PROMPT)
        lib.amd_set_constraint(ctx, 0, h)
        lib.amd_conversation_seed(ctx, 0, 5, 3)
        lib.amd_logits(ctx)
        ids, n, nxt, st = np.zeros(8, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(4, np.int32)
        ip = lambda x: x.ctypes.data_as(I32P) if x is not None else None

        def verify(draft=(7, 8), n_draft=None, temp=0.8, top_k=40, top_p=0.9, ids=ids, n=n, nxt=nxt, null_draft=False):
            d = np.array(draft, np.int32)
            return L.minigpt4_amd_verify_draft_sampled(ctx.ptr, None if null_draft else ip(d), len(d) if n_draft is None else n_draft, temp, top_k, top_p, ip(ids), ip(n), ip(nxt),
                                                       None, None)

        def lookup(corpus=(7, 8), max_tokens=4, ngram_max=3, ngram_min=1, n_draft=2, temp=0.8, top_k=40, top_p=0.9, out=ids, n=n, st=st):
            c = np.array(corpus, np.int32)
            return L.minigpt4_amd_decode_lookup_sampled(ctx.ptr, ip(c), len(c), max_tokens, ngram_max, ngram_min, n_draft, temp, top_k, top_p, ip(out), ip(n), ip(st))
        before = _snapshot(lib, ctx, 0)
        assert before["spec"] == dict.fromkeys(lib.SPECULATION_INFO_FIELDS, 0)
        lib.amd_select_conversation(ctx, 0)
        for f, name in ((verify, b"verify_draft_sampled: "), (lookup, b"decode_lookup_sampled: ")):    # speculation off
            assert f() == 1 and L.minigpt4_amd_last_error().startswith(name) and b"speculation is off" in L.minigpt4_amd_last_error()
        lib.amd_set_speculation(ctx, 3)
        common = (dict(temp=0.0), dict(temp=-0.5), dict(temp=float("nan")), dict(temp=float("inf")), dict(top_k=0), dict(top_k=65), dict(top_k=-3), dict(top_p=0.0),
                  dict(top_p=1.0001), dict(top_p=float("nan")), dict(n=None))
        for kw in common + (dict(n_draft=-1), dict(draft=(7, 8, 9, 10)), dict(null_draft=True, n_draft=2), dict(draft=(7, 512)), dict(draft=(-1,)), dict(ids=None), dict(nxt=None)):
            assert verify(**kw) == 1, kw
            assert L.minigpt4_amd_last_error().startswith(b"verify_draft_sampled: "), (kw, L.minigpt4_amd_last_error())
        for kw in common + (dict(n_draft=0), dict(n_draft=4), dict(corpus=(7, 512)), dict(max_tokens=0), dict(ngram_min=0), dict(ngram_max=0), dict(out=None), dict(st=None)):
            assert lookup(**kw) == 1, kw
            assert L.minigpt4_amd_last_error().startswith(b"decode_lookup_sampled: "), (kw, L.minigpt4_amd_last_error())
        assert L.minigpt4_amd_speculation_info(ctx.ptr, None) == 1 and L.minigpt4_amd_last_error().startswith(b"speculation_info: ")
        lib.amd_select_conversation(ctx, 1)                                      # nothing queued, nothing evaluated
        for f, name in ((verify, b"verify_draft_sampled: "), (lookup, b"decode_lookup_sampled: ")):
            assert f() == 1 and L.minigpt4_amd_last_error().startswith(name) and b"no current logits" in L.minigpt4_amd_last_error()
        assert _same(_snapshot(lib, ctx, 0), before)
        # "context full" is refused before a draw is counted: conversation 2 filled to the last row, no automatic shift
        lib.amd_select_conversation(ctx, 2)
        lib.minigpt4_begin_chat(ctx, PROMPT)
        lib.amd_logits(ctx)
        room = 96 - _n_past(lib, ctx, 2)
        lib.amd_select_conversation(ctx, 2)
        lib.amd_eval_tokens(ctx, [5 + (7 * i) % 200 for i in range(room)])
        lib.amd_conversation_seed(ctx, 2, 77, 11)
        full = _snapshot(lib, ctx, 2)
        assert full["p"] == 96
        lib.amd_select_conversation(ctx, 2)
        assert verify() == 1
        assert L.minigpt4_amd_last_error().startswith(b"verify_draft_sampled: context full"), L.minigpt4_amd_last_error()   # (the wrapper appends the test library's own last text)
        assert _same(_snapshot(lib, ctx, 2), full) and full["draws"] == 11 and full["spec"]["launches"] == 0
        lib.amd_select_conversation(ctx, 2)
        assert lookup() == 0 and n[0] == 0 and st.tolist() == [0, 0, 0, 0]          # the loop ends on a full context that cannot shift: nothing emitted, no draw
        assert _same(_snapshot(lib, ctx, 2), full)
        # with room for x0 only, the draft is cut to the room left
        lib.amd_select_conversation(ctx, 0)
        lib.amd_eval_tokens(ctx, [3 + 0x30 + i % 10 for i in range(95 - before["p"])])
        lib.amd_select_conversation(ctx, 0)
        r = lib.amd_verify_draft_sampled(ctx, [3 + 0x35, 3 + 0x36], want_rows=True)
        assert len(r["ids"]) == 1 and r["row_sampled"][0] >= 0 and (r["row_sampled"][1:] == -1).all() and _n_past(lib, ctx, 0) == 96
        assert lib.amd_sampling_info(ctx, 0)["draws"] == 4 and lib.amd_speculation_info(ctx)["sent"] == 0
    finally:
        lib.minigpt4_free(ctx)


@gpu
def test_the_greedy_verify_pass_is_what_it_was(gpu_lib, tiny_files):
    """The greedy verify_draft gives the same ids and logits before and after sampled calls on the same context (its captured passes survive them), and a context that
    uses greedy speculation and the sampled batched step but never the new entry points reports zero."""
    lib = gpu_lib
    ctx = _load(lib, tiny_files, 4)
    try:
        lib.minigpt4_begin_chat(ctx, PROMPT)
        lib.amd_fork_conversation(ctx, 0, [1, 2, 3])
        lib.amd_select_conversation(ctx, 3)
        g = [int(t) for t in lib.amd_decode_lookup(ctx, [], 6, n_draft=1)["tokens"]]        # the greedy continuation
        draft = [g[1], g[2], (g[3] + 1) % 512, g[4]]
        lib.amd_select_conversation(ctx, 1)
        first = lib.amd_verify_draft(ctx, draft)
        row1 = lib.amd_logits(ctx).copy()
        lib.amd_end_chat_batch_sampled(ctx, [3], *PARAMS[0])
        assert lib.amd_speculation_info(ctx) == dict.fromkeys(lib.SPECULATION_INFO_FIELDS, 0)
        lib.amd_select_conversation(ctx, 0)
        for d in ([], draft, draft[:2], draft):
            lib.amd_verify_draft_sampled(ctx, d, *PARAMS[0])
        assert lib.amd_speculation_info(ctx)["passes"] == 4
        lib.amd_select_conversation(ctx, 2)
        second = lib.amd_verify_draft(ctx, draft)
        assert first["ids"].tolist() == second["ids"].tolist() == g[:3] and first["row_greedy"].tolist() == second["row_greedy"].tolist()
        assert np.array_equal(lib.amd_logits(ctx), row1)
    finally:
        lib.minigpt4_free(ctx)
