"""The extended device-side sampling rule on the device (include/minigpt4_amd.h: tail-free, typical, top-p, min-p over the live list; mirostat v2 with one mu per
conversation): k_sample_rows_ex alone through minigpt4_amd_test_sample_rows_ex against tests/sampler_chain_ref.py's float64 restatement, then
minigpt4_amd_end_chat_batch_sampled_ex / _sampled_candidates_ex / _conversation_mirostat / _mirostat_info on the tiny model files of tests/test_gpu_device_sampling.py,
then the server.

The new code acts on at most 64 candidates in LDS and the selection is covered at 32 001 ids by tests/test_gpu_device_sampling.py, so the shapes are its small ones; top_k
in {1, 2, 3, 40, 64} makes n_c hit 1, 2, 3, the default and the cap.  Exact: candidate ids, n_cand, the Philox word, the stuck flag, the row tokens; with neutral
parameters every output word equals k_sample_rows' of the same launch inputs.  p_j within 2e-4 relative of float64 (|w| <= 64 here, as that file requires).  The live list,
the pick and mirostat's cut are compared exactly except where the float64 reference ALONE finds a threshold too close -- sampler_chain_ref.py derives each margin from the
error behind the 2e-4 bound; tail-free's scales with 1 / s, so the rows are peaked (the top logit raised by 1.5) -- and such a decision must still be an admissible
neighbour, from which the reference is continued.  Caps for the random rows: 5 % of a case's rows, 1 % of its draws (checked on the CPU first with
minigpt4_amd_test_sample_chain on the same rows; a seed that exceeds a cap is changed, never the cap).  Mirostat sequences are teacher-forced: the kernel's mu' starts the
next decision on both sides, so rounding cannot accumulate into another cut.  mu' within the bound sampler_chain_ref.judge_mirostat derives from the error of p_pick.
Last, draft verification under the extended rule (minigpt4_amd_verify_draft_sampled_ex / _decode_lookup_sampled_ex): in parity mode the lookup loop emits the plain _ex
loop's tokens one for one; in fast mode every row of the one-pass form is sampled by the rule on its own logits."""
import ctypes
import os

import numpy as np
import pytest

import sampler_chain_ref as CR
import sampling_ref as SR
from test_gpu_device_sampling import (N_CTX, PAD, PROMPT, _hist, _load, _n_past, _prompt, _reference, _row, _setup, f32_word, random_specs, spec)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 100, 100), (3, 512, 512), (5, 513, 520), (2, 64, 72)]
TOP_K = (1, 2, 3, 40, 64)
NEUTRAL = dict(tfs_z=1.0, typical_p=1.0, min_p=0.0)
SETS = [("neutral", 0.8, 0.9, NEUTRAL), ("neutral_all", 1.5, 1.0, NEUTRAL), ("tail_free", 0.8, 1.0, dict(NEUTRAL, tfs_z=0.95)), ("typical", 1.0, 1.0, dict(NEUTRAL, typical_p=0.9)),
        ("min_p", 0.8, 0.9, dict(NEUTRAL, min_p=0.05)), ("all_four", 0.8, 0.9, dict(tfs_z=0.95, typical_p=0.9, min_p=0.05)), ("tight", 0.25, 0.5, dict(tfs_z=0.5, typical_p=0.3, min_p=0.4))]
N_DRAWS = 4
MIRO = [(0.8, 5.0, 0.1), (1.0, 3.0, 0.3), (1.5, 2.0, 1.0)]                    # (temp, tau, eta)


def _buffer(rng, rows, V, ld):
    buf = np.full((rows, ld), PAD, np.float32)
    buf[:, :V] = 3.0 * rng.standard_normal((rows, V)).astype(np.float32)
    for r in range(rows):
        buf[r, int(np.argmax(buf[r, :V]))] += np.float32(1.5)                  # peaked rows: tail-free's s, and with it its margin, stays in hand
    return buf


def _descriptors(specs, combos, n_draws):
    """one descriptor per (spec, combo, draw); combos = [(temp, top_p, top_k, chain row of 7)].  (rows, table, bitmaps, bm_of, seed_draws, params, top_k, chain, key)"""
    rows, table, bitmaps, bm_of, seed_draws, params, top_k, chain, key = [], [], [], [], [], [], [], [], []
    for s_i, sp in enumerate(specs):
        off = len(table)
        table += [(t, c, f32_word(b), hb) for t, c, b, hb in sp["table"]]
        if sp["bitmap"] is not None:
            bitmaps.append(sp["bitmap"])
        pen = sp["pen"]
        for c_i, (temp, top_p, k, ch) in enumerate(combos):
            for d in range(n_draws):
                rows.append((sp["row"], off, len(sp["table"]), pen["flags"], f32_word(pen["repeat_penalty"]), f32_word(pen["alpha_frequency"]), f32_word(pen["alpha_presence"]), 0))
                bm_of.append(len(bitmaps) - 1 if sp["bitmap"] is not None else -1)
                seed_draws.append(((2000 + 7 * s_i) | (s_i << 32), (c_i * n_draws + d) * 0x9E37 + (1 << 40 if d % 4 == 3 else 0)))
                params.append((temp, top_p)); top_k.append(k); chain.append(ch); key.append((s_i, c_i, d))
    return rows, table, bitmaps, bm_of, seed_draws, params, top_k, chain, key


def _launch(lib, buf, V, desc, ex=True, tok=None):
    rows, table, bitmaps, bm_of, seed_draws, params, top_k, chain, _ = desc
    args = (buf, V, np.array(rows, np.int32), np.array(table, np.int64).astype(np.int32).reshape(-1, 4), params, top_k, np.array(seed_draws, np.uint64))
    kw = dict(bitmaps=np.array(bitmaps, np.uint32) if bitmaps else None, bitmap_of_row=bm_of, tok_index=tok)
    return lib.amd_test_sample_rows_ex(*args, chain, **kw) if ex else lib.amd_test_sample_rows(*args, **kw)


def _words(seed_draws):
    sd = np.array(seed_draws, np.uint64)
    return SR.philox4x32_10(np.stack([sd[:, 1] & 0xFFFFFFFF, sd[:, 1] >> np.uint64(32), 0 * sd[:, 1], 0 * sd[:, 1]], -1), np.stack([sd[:, 0] & 0xFFFFFFFF, sd[:, 0] >> np.uint64(32)], -1))[:, 0]


def _candidates(buf, V, sp, top_k):
    trow = SR.transformed(buf[sp["row"], :V], sp["table"], sp["pen"])
    return SR.candidates(trow, top_k, None if sp["bitmap"] is None else SR.bitmap_ids(sp["bitmap"], V))


def _decision(got, d, ids):
    """descriptor d of a launch as the judges take it: the pick as a candidate index"""
    n_c = len(ids)
    return dict(pick=int(np.nonzero(ids == got["pick"][d])[0][0]), kept=int(got["kept"][d]), p=got["p"][d][:n_c], mask=int(got["mask"][d]), mu=got["mu"][d], observed=got["observed"][d])


def _exact_part(got, d, ids, word, tag):
    n_c = len(ids)
    assert got["word"][d] == word and got["n_cand"][d] == n_c, tag
    assert np.array_equal(got["ids"][d][:n_c], ids) and (got["ids"][d][n_c:] == -1).all(), tag
    if n_c == 0:                                                             # nothing takes part: "</s>", flagged, an empty live list
        assert got["stuck"][d] == 1 and got["pick"][d] == SR.EOS and got["kept"][d] == 0 and (got["p"][d] == 0).all() and got["mask"][d] == 0 and got["observed"][d] == 0, tag
        return False
    assert got["stuck"][d] == 0, tag
    return True


@pytest.mark.parametrize("k,shape", list(enumerate(SHAPES)), ids=lambda v: "r%d_v%d_ld%d" % v if isinstance(v, tuple) else None)
def test_kernel_filters_against_float64(gpu_lib, k, shape):
    n_buf, V, ld = shape
    rng = np.random.default_rng(500 + k)
    buf = _buffer(rng, n_buf, V, ld)
    specs = random_specs(rng, buf, V) + [spec(0, bitmap=SR.make_bitmap(V, []))]   # and a row where no id takes part
    combos = [(temp, top_p, min(tk, V), [kw["tfs_z"], kw["typical_p"], kw["min_p"], 0, 5.0, 0.1, 3.25]) for _, temp, top_p, kw in SETS for tk in TOP_K]
    desc = _descriptors(specs, combos, N_DRAWS)
    n = len(desc[0])
    tok = np.array([d if d < 48 else -1 for d in range(n)], np.int32)
    got = _launch(gpu_lib, buf, V, desc, tok=tok)
    words = _words(desc[4])
    cands = {}
    n_rows = bad_rows = n_draws = bad_draws = 0
    row_ex = {}
    for d, (s_i, c_i, dr) in enumerate(desc[8]):
        name, temp, top_p, kw = SETS[c_i // len(TOP_K)]
        tk = combos[c_i][2]
        if (s_i, tk) not in cands:
            cands[(s_i, tk)] = _candidates(buf, V, specs[s_i], tk)
        ids, vals = cands[(s_i, tk)]
        tag = (shape, name, tk, s_i, dr)
        assert got["mu"][d] == np.float32(3.25), tag                         # mirostat 0: mu as given
        if not _exact_part(got, d, ids, words[d], tag):
            continue
        ex, near_u = CR.judge_chain(_decision(got, d, ids), vals, temp, top_p, int(words[d]), **kw)
        row_ex[(s_i, c_i)] = row_ex.get((s_i, c_i), False) or ex
        n_draws += 1
        bad_draws += near_u
    n_rows, bad_rows = len(row_ex), sum(row_ex.values())
    for d in range(n):                                                       # the hand-over: written where an index was given, nowhere else
        if tok[d] >= 0:
            assert got["row_tok"][tok[d]] == got["pick"][d], d
    assert (got["row_tok"][min(n, 48):] == -7).all()
    # neutral parameters: every word of the plain kernel's output, bit for bit, from the same launch inputs
    neutral = [c_i for c_i in range(len(combos)) if SETS[c_i // len(TOP_K)][3] == NEUTRAL]
    sel = [d for d, (_, c_i, _) in enumerate(desc[8]) if c_i in neutral]
    sub = tuple([x[d] for d in sel] if i in (0, 3, 4, 5, 6, 7, 8) else x for i, x in enumerate(desc))
    plain = _launch(gpu_lib, buf, V, sub, ex=False)
    for f in ("pick", "stuck", "word", "n_cand", "kept", "ids"):
        assert np.array_equal(plain[f], got[f][sel]), f
    assert np.array_equal(plain["p"].view(np.uint32), got["p"][sel].view(np.uint32))
    assert all(int(got["mask"][d]) == (1 << int(got["kept"][d])) - 1 for d in sel)
    print(f"shape {shape}: {n} decisions in one launch ({got['ms'] * 1e3:.0f} us), {bad_rows} of {n_rows} rows and {bad_draws} of {n_draws} draws excluded")
    assert bad_rows <= 0.05 * n_rows and bad_draws <= 0.01 * n_draws, (bad_rows, n_rows, bad_draws, n_draws)


@pytest.mark.parametrize("k,shape", list(enumerate(SHAPES)), ids=lambda v: "r%d_v%d_ld%d" % v if isinstance(v, tuple) else None)
def test_kernel_mirostat_sequences_against_float64(gpu_lib, k, shape):
    n_buf, V, ld = shape
    rng = np.random.default_rng(600 + k)
    buf = _buffer(rng, n_buf, V, ld)
    specs = random_specs(rng, buf, V) + [spec(0, bitmap=SR.make_bitmap(V, []))]
    base = [(temp, 0.9, min(tk, V), [0.5, 0.5, 0.5, 2, tau, eta, float("nan")]) for temp, tau, eta in MIRO for tk in TOP_K]   # the filters' values are ignored
    mu = {}                                                                  # (spec, combo) -> the kernel's mu' of the step before; none: unset
    rows = set()
    bad_rows, n_draws, bad_draws = set(), 0, 0
    for step in range(6):
        desc = _descriptors(specs, base, 1)
        for d, (s_i, c_i, _) in enumerate(desc[8]):
            desc[4][d] = (desc[4][d][0], desc[4][d][1] + step)                 # the next draw of the same stream
            desc[7][d] = list(desc[7][d][:6]) + [mu.get((s_i, c_i), float("nan"))]
        got = _launch(gpu_lib, buf, V, desc)
        words = _words(desc[4])
        for d, (s_i, c_i, _) in enumerate(desc[8]):
            temp, _, tk, ch = base[c_i]
            tau, eta = ch[4], ch[5]
            ids, vals = _candidates(buf, V, specs[s_i], tk)
            tag = (shape, step, s_i, c_i)
            start = mu.get((s_i, c_i))
            if not _exact_part(got, d, ids, words[d], tag):
                assert got["mu"][d] == np.float32(2 * tau if start is None else start), tag   # stuck: mu as a decision finds it, not moved
                mu[(s_i, c_i)] = float(got["mu"][d])
                continue
            ex, near_u = CR.judge_mirostat(_decision(got, d, ids), vals, temp, int(words[d]), tau, eta, start)
            rows.add((s_i, c_i))
            if ex:
                bad_rows.add((s_i, c_i))
            n_draws += 1
            bad_draws += near_u
            mu[(s_i, c_i)] = float(got["mu"][d])
    print(f"shape {shape}: 6 teacher-forced steps, {len(bad_rows)} of {len(rows)} rows and {bad_draws} of {n_draws} draws excluded")
    assert len(bad_rows) <= 0.05 * len(rows) and bad_draws <= 0.01 * n_draws


# ------------------------------------------------------------------------------------------------ the engine
PARAMS = (0.8, 40, 0.9)
FILTERS = [dict(tfs_z=0.95), dict(typical_p=0.9), dict(min_p=0.05), dict(tfs_z=0.95, typical_p=0.9, min_p=0.05)]
MIRO_KW = dict(mirostat=2, mirostat_tau=3.0, mirostat_eta=0.3)


def _cand_state(lib, ctx, slots):
    return [(_n_past(lib, ctx, s), _hist(lib, ctx, s), lib.amd_sampling_info(ctx, s)["draws"], lib.amd_mirostat_info(ctx, s)["mu"]) for s in slots]


def test_neutral_ex_step_equals_the_plain_step(gpu_lib, tiny_files):
    lib = gpu_lib
    a, b = _load(lib, tiny_files, 4), _load(lib, tiny_files, 4)
    slots = [1, 3, 0, 2]
    try:
        ha, hb = lib.amd_constraint_compile(a, r"[0-9]+"), lib.amd_constraint_compile(b, r"[0-9]+")
        _setup(lib, a, ha, full_slot=3)
        _setup(lib, b, hb, full_slot=3)
        for step in range(16):
            ca, cb = lib.amd_sampled_candidates(a, slots, *PARAMS, _extended=True), lib.amd_sampled_candidates(b, slots, *PARAMS)
            assert np.array_equal(ca["ids"], cb["ids"]) and np.array_equal(ca["probs"].view(np.uint32), cb["probs"].view(np.uint32)), step
            assert np.array_equal(ca["n_cand"], cb["n_cand"]) and np.array_equal(ca["kept"], cb["kept"]), step
            assert all(int(m) == (1 << int(k)) - 1 for m, k in zip(ca["kept_mask"], cb["kept"])), step
            ia = lib.amd_end_chat_batch_sampled(a, slots, *PARAMS, with_ids=True, _extended=True)
            ib = lib.amd_end_chat_batch_sampled(b, slots, *PARAMS, with_ids=True)
            assert ia[0] == ib[0] and np.array_equal(ia[1], ib[1]), step
            for s in slots:
                assert lib.amd_sampling_info(a, s)["draws"] == lib.amd_sampling_info(b, s)["draws"] == step + 1
                assert np.array_equal(_row(lib, a, s), _row(lib, b, s)) and _hist(lib, a, s) == _hist(lib, b, s), (step, s)
                assert lib.amd_mirostat_info(a, s)["set"] is False
        x, y = lib.amd_sampling_info(a, 0), lib.amd_sampling_info(b, 0)
        assert (x["launches"], x["handed"], x["rows"], x["stuck"]) == (y["launches"], y["handed"], y["rows"], y["stuck"]) and x["launches"] == 32   # the _ex calls are counted
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


def _pick_from_report(c, i, word):
    """the draw of step 5 over the probabilities sampled_candidates_ex reported for entry i: (candidate index, near a boundary)"""
    L = [j for j in range(64) if int(c["kept_mask"][i]) >> j & 1]
    cum = np.cumsum(c["probs"][i][L].astype(np.float64))
    cum /= cum[-1]
    u = float(word >> 8) * 2.0 ** -24
    above = np.nonzero(cum > u)[0]
    return L, (int(above[0]) if len(above) else len(L) - 1), bool(len(L) > 1 and np.abs(cum[:-1] - u).min() < CR.MARGIN)


@pytest.mark.parametrize("f_i", range(len(FILTERS)))
def test_filtered_step_equals_the_rule_and_a_forced_twin(gpu_lib, tiny_files, f_i):
    lib, kw = gpu_lib, FILTERS[f_i]
    a, b = _load(lib, tiny_files, 4), _load(lib, tiny_files, 4)
    slots = [1, 3, 0, 2]
    try:
        h = lib.amd_constraint_compile(a, r"[0-9]+")
        _setup(lib, a, h, full_slot=3)
        _setup(lib, b, 0, full_slot=3)
        cut = 0
        for step in range(6):
            state = lib.amd_constraint_info(a, 2)["state"]
            refs = [_reference(lib, a, s, PARAMS, h, state) for s in slots]
            before = _cand_state(lib, a, slots)
            c = lib.amd_sampled_candidates(a, slots, *PARAMS, **kw)
            assert _cand_state(lib, a, slots) == before                      # nothing advanced, no draw counted
            past0 = [_n_past(lib, a, s) for s in slots]
            pcs, ids = lib.amd_end_chat_batch_sampled(a, slots, *PARAMS, with_ids=True, **kw)
            for i, s in enumerate(slots):
                cand_ids, vals = refs[i]
                n_c = len(cand_ids)
                assert c["n_cand"][i] == n_c and np.array_equal(c["ids"][i][:n_c], cand_ids), (step, s)
                word = SR.draw_word(1337 | (s << 32), step)
                L, at, near = _pick_from_report(c, i, word)
                j = int(np.nonzero(cand_ids == ids[i])[0][0])
                assert j in L and (abs(L.index(j) - at) <= 1 if near else L.index(j) == at), (step, s, j, L, at)
                CR.judge_chain(dict(pick=j, kept=int(c["kept"][i]), p=c["probs"][i][:n_c], mask=int(c["kept_mask"][i])), vals, PARAMS[0], PARAMS[2], word, **kw)
                cut += int(c["kept_mask"][i]) != (1 << n_c) - 1
                assert pcs[i] == lib.amd_token_piece(a, int(ids[i])) and lib.amd_sampling_info(a, s)["draws"] == step + 1
            lib.amd_eval_batch(b, slots, [int(t) for t in ids])
            for i, s in enumerate(slots):
                assert _n_past(lib, a, s) == _n_past(lib, b, s) == past0[i] + (0 if s == 3 else 1), (step, s)
                assert np.array_equal(_row(lib, a, s), _row(lib, b, s)) and _hist(lib, a, s) == _hist(lib, b, s), (step, s)
        assert cut > 0                                                       # the filters did shorten lists
    finally:
        lib.minigpt4_free(a)
        lib.minigpt4_free(b)


def test_mu_belongs_to_the_conversation(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _load(lib, tiny_files, 4)
    slots = [0, 3, 1]
    tau, eta = MIRO_KW["mirostat_tau"], MIRO_KW["mirostat_eta"]
    try:
        _setup(lib, ctx, 0, full_slot=3)
        assert all(lib.amd_mirostat_info(ctx, s) == dict(set=False, mu=None, observed=0, tau=0) for s in range(4))
        mu = {s: None for s in slots}
        for step in range(4):
            refs = [_reference(lib, ctx, s, PARAMS) for s in slots]
            c = lib.amd_sampled_candidates(ctx, slots, *PARAMS, **MIRO_KW)
            assert [lib.amd_mirostat_info(ctx, s)["mu"] for s in slots] == [mu[s] for s in slots]   # the report moves no mu (an unset one stays unset)
            past3 = _n_past(lib, ctx, 3)
            ids = lib.amd_end_chat_batch_sampled(ctx, slots, *PARAMS, with_ids=True, **MIRO_KW)[1]
            assert _n_past(lib, ctx, 3) == past3 == N_CTX                    # the full conversation is sampled, not advanced ...
            for i, s in enumerate(slots):
                cand_ids, vals = refs[i]
                info = lib.amd_mirostat_info(ctx, s)
                assert info["set"] and info["tau"] == np.float32(tau), (step, s)   # ... and its mu moves like the others'
                j = int(np.nonzero(cand_ids == ids[i])[0][0])
                n = int(c["kept"][i])
                got = dict(pick=j, kept=n, p=c["probs"][i][:len(vals)], mask=int(c["kept_mask"][i]), mu=info["mu"], observed=info["observed"])
                CR.judge_mirostat(got, vals, PARAMS[0], SR.draw_word(1337 | (s << 32), step), tau, eta, mu[s])
                if step == 0:                                                # unset: the decision started from 2 * tau
                    want = CR.mirostat64(vals, PARAMS[0], 0, tau, eta, None, n=n, at=j)
                    assert want["mu_in"] == 2 * tau and abs(float(info["mu"]) - want["mu"]) < 1e-3
                mu[s] = float(info["mu"])
        lib.amd_select_conversation(ctx, 0)
        lib.minigpt4_reset_chat(ctx)
        assert lib.amd_mirostat_info(ctx, 0)["mu"] == np.float32(mu[0])      # reset_chat leaves the sampler's state alone
        lib.amd_conversation_mirostat(ctx, 1, 4.5)
        assert lib.amd_mirostat_info(ctx, 1)["mu"] == np.float32(4.5)
        lib.amd_conversation_mirostat(ctx, 1, None)
        assert lib.amd_mirostat_info(ctx, 1)["set"] is False
        assert lib.amd_sampling_info(ctx, 0)["launches"] == 8
        lib.amd_set_conversations(ctx, 4)
        assert all(lib.amd_mirostat_info(ctx, s)["set"] is False for s in range(4))
    finally:
        lib.minigpt4_free(ctx)


def test_mirostat_does_not_depend_on_the_company(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _load(lib, tiny_files, 4, n_ctx=256, conditioned=False)
    try:
        lib.amd_set_parity(ctx, True)
        runs = []
        for slot, listing in ((0, [0]), (0, [2, 0, 1]), (2, [1, 2, 3])):         # alone, with two others, in another slot
            for s in listing:
                _prompt(lib, ctx, s, PROMPT if s == slot else f"partner {s} of {len(listing)}")
                lib.amd_conversation_seed(ctx, s, 4242 if s == slot else 17 + s, 0)
                lib.amd_conversation_mirostat(ctx, s, None)
            ids, mus = [], []
            for _ in range(16):
                ids.append(int(lib.amd_end_chat_batch_sampled(ctx, listing, 0.8, 40, 0.9, with_ids=True, **MIRO_KW)[1][listing.index(slot)]))
                mus.append(lib.amd_mirostat_info(ctx, slot)["mu"])
            runs.append((ids, np.array(mus, np.float32).view(np.uint32).tolist()))
        assert runs[0] == runs[1] == runs[2], runs
        assert len(set(runs[0][0])) > 1 and len(set(runs[0][1])) > 1
    finally:
        lib.minigpt4_free(ctx)


def test_refusals_leave_everything_untouched(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _load(lib, tiny_files, 4)
    I32P = ctypes.POINTER(ctypes.c_int32)
    L = lib.library
    try:
        for s in (0, 1):
            _prompt(lib, ctx, s, PROMPT)
        lib.amd_select_conversation(ctx, 0)
        lib.amd_logits(ctx)
        lib.amd_conversation_mirostat(ctx, 0, 2.5)
        toks, ids = (ctypes.c_char_p * 4)(), np.zeros(4 * 64, np.int32)
        ok = dict(temp=0.8, top_k=40, top_p=0.9, tfs_z=1.0, typical_p=1.0, min_p=0.0, mirostat=0, tau=5.0, eta=0.1)

        def step(slots, **kw):
            p, sl = {**ok, **kw}, np.array(slots, np.int32)
            return L.minigpt4_amd_end_chat_batch_sampled_ex(ctx.ptr, sl.ctypes.data_as(I32P) if len(sl) else None, len(sl), toks, p["temp"], p["top_k"], p["top_p"], p["tfs_z"],
                                                            p["typical_p"], p["min_p"], p["mirostat"], p["tau"], p["eta"], ids.ctypes.data_as(I32P))

        def cand(slots, **kw):
            p, sl = {**ok, **kw}, np.array(slots, np.int32)
            return L.minigpt4_amd_sampled_candidates_ex(ctx.ptr, sl.ctypes.data_as(I32P) if len(sl) else None, len(sl), p["temp"], p["top_k"], p["top_p"], p["tfs_z"],
                                                        p["typical_p"], p["min_p"], p["mirostat"], p["tau"], p["eta"], ids.ctypes.data_as(I32P), None, None, None)
        before = [(_n_past(lib, ctx, s), lib.amd_sampling_info(ctx, s), lib.amd_mirostat_info(ctx, s)) for s in range(4)]
        nan, inf = float("nan"), float("inf")
        for f, name in ((step, b"end_chat_batch_sampled_ex: "), (cand, b"sampled_candidates_ex: ")):
            for slots, kw in (([], {}), ([0, 0], {}), ([0, 4], {}), ([0], dict(temp=0.0)), ([0], dict(top_k=65)), ([0], dict(top_p=nan)),
                              ([0], dict(tfs_z=0.0)), ([0], dict(tfs_z=1.5)), ([0], dict(tfs_z=nan)), ([0], dict(typical_p=0.0)), ([0], dict(typical_p=1.01)), ([0], dict(typical_p=nan)),
                              ([0], dict(min_p=-0.1)), ([0], dict(min_p=1.1)), ([0], dict(min_p=nan)), ([0], dict(mirostat=1)), ([0], dict(mirostat=3)), ([0], dict(mirostat=-2)),
                              ([0], dict(tau=0.0)), ([0], dict(tau=inf)), ([0], dict(tau=nan)), ([0], dict(eta=-0.5)), ([0], dict(eta=inf)), ([0], dict(eta=nan)),
                              ([0, 2], {})):                                   # conversation 2 has nothing queued and nothing evaluated
                assert f(slots, **kw) == 1, (name, slots, kw)
                assert L.minigpt4_amd_last_error().startswith(name), L.minigpt4_amd_last_error()
            # (the binding's error text is the product library's, then " | " and the test library's own, once a hook has left one there: the refusal is the first part)
            assert f([0], mirostat=1) == 1 and L.minigpt4_amd_last_error().split(b" | ")[0] == name + b"mirostat v1 is not built"
        assert L.minigpt4_amd_conversation_mirostat(ctx.ptr, 4, 1.0) == 1 and L.minigpt4_amd_last_error().startswith(b"conversation_mirostat: ")
        assert L.minigpt4_amd_conversation_mirostat(ctx.ptr, 0, inf) == 1 and L.minigpt4_amd_last_error().startswith(b"conversation_mirostat: ")
        assert L.minigpt4_amd_mirostat_info(ctx.ptr, -1, np.zeros(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 1
        assert L.minigpt4_amd_mirostat_info(ctx.ptr, 0, None) == 1 and L.minigpt4_amd_last_error().startswith(b"mirostat_info: ")
        assert [(_n_past(lib, ctx, s), lib.amd_sampling_info(ctx, s), lib.amd_mirostat_info(ctx, s)) for s in range(4)] == before
        assert before[0][1]["launches"] == 0 and before[0][2]["mu"] == np.float32(2.5)   # nothing was launched
        assert step([0, 1], top_k=64, top_p=1.0, min_p=1.0) == 0               # the ends of the ranges are inside them
        assert lib.amd_sampling_info(ctx, 0)["draws"] == 1 and lib.amd_mirostat_info(ctx, 0)["mu"] == np.float32(2.5)   # mirostat 0 moves no mu
    finally:
        lib.minigpt4_free(ctx)


def test_server_mirostat_gives_each_request_the_text_it_gets_alone(gpu_lib, tmpdir_models):
    from minigpt4_cpp_amd import modelgen as G, serve as S
    vp, lp = os.path.join(tmpdir_models, "vision_serve_chain.bin"), os.path.join(tmpdir_models, "llm_serve_chain.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=31, std=0.05)                       # tests/test_gpu_serve.py's model
    G.write_llm_file(lp, G.tiny_llm(wtype="q4_0", n_embd=4096, n_layer=1, n_head=32, n_vocab=512, output_type="q6_k"), seed=4, std=0.02)
    reqs = [S.Request(G.synth_image(3 + i), p, 10) for i, p in enumerate(["what is the text in the picture?", "describe it", "colour?"])]
    seeds = [11, 22, 33]
    srv = S.ReplicaServer(vp, lp, conversations=2, n_ctx=512, n_batch=64, library=gpu_lib)           # waves of 2 + 1
    try:
        srv.lib.amd_set_parity(srv.ctx, True)                                # logits that do not depend on the batch: the text depends on the seed and the request's own mu
        kw = dict(temp=0.8, top_k=40, top_p=0.9, ignore_eos=True, device_sampling=True, mirostat=2, mirostat_tau=3.0, mirostat_eta=0.3)
        together = srv.run(reqs, seeds=seeds, **kw)
        assert srv.run([reqs[1]], seeds=[seeds[1]], **kw) == [together[1]]     # alone, in slot 0 instead of slot 1, after a request that left its mu there
        assert srv.run(reqs[::-1], seeds=seeds[::-1], **kw) == together[::-1]  # other partners, other slots
        assert len(set(together)) == 3 and all(together)
        assert srv.lib.amd_mirostat_info(srv.ctx, 0)["set"]
        filt = {**kw, **dict(mirostat=0, tfs_z=0.95, typical_p=0.9, min_p=0.05)}
        assert srv.run([reqs[2]], seeds=[seeds[2]], **filt) == [srv.run(reqs, seeds=seeds, **filt)[2]]
    finally:
        srv.close()


# ------------------------------------------------------------------------------------------------ draft verification under the extended rule
SPEC_KW = dict(tfs_z=0.95, typical_p=0.9, min_p=0.05)


def _spec_ctx(lib, tiny_files, parity):
    import test_gpu_draft_sampled as DS
    ctx = DS._load(lib, tiny_files, 2, parity=parity, max_draft=4)
    lib.minigpt4_begin_chat(ctx, DS.PROMPT)
    lib.amd_conversation_seed(ctx, 0, 99, 5)
    lib.amd_fork_conversation(ctx, 0, [1])
    lib.amd_conversation_seed(ctx, 1, 99, 5)
    return ctx


def test_parity_lookup_ex_equals_the_plain_ex_loop(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _spec_ctx(lib, tiny_files, parity=True)
    try:
        plain = [int(lib.amd_end_chat_batch_sampled(ctx, [1], *PARAMS, with_ids=True, **SPEC_KW)[1][0]) for _ in range(24)]
        if SR.EOS in plain:
            plain = plain[:plain.index(SR.EOS) + 1]                          # the lookup loop ends behind "</s>"; the plain loop does not know it
        lib.amd_select_conversation(ctx, 0)
        before = lib.amd_speculation_info(ctx)
        r = lib.amd_decode_lookup_sampled(ctx, plain, 24, ngram_max=3, ngram_min=1, n_draft=4, temp=PARAMS[0], top_k=PARAMS[1], top_p=PARAMS[2], **SPEC_KW)   # the corpus: the text itself
        got = [int(t) for t in r["tokens"]]
        assert got == plain, (got, plain)                                    # token for token
        assert r["passes"] + r["steps"] + r["accepted"] == len(got)
        assert r["passes"] > 0 and r["accepted"] > 0 and r["sent"] >= r["accepted"], r   # the drafter fired and its drafts were kept
        assert lib.amd_sampling_info(ctx, 0)["draws"] == 5 + len(got)
        assert _hist(lib, ctx, 0) == _hist(lib, ctx, 1)[:len(_hist(lib, ctx, 0))]
        if len(got) == 24:
            assert np.array_equal(_row(lib, ctx, 0), _row(lib, ctx, 1))      # oracle-order passes: the same logits bit for bit
        info = lib.amd_speculation_info(ctx)                                 # the _ex calls are counted
        assert info["accepted"] - before["accepted"] == r["accepted"] and info["sent"] - before["sent"] == r["sent"] and info["passes"] - before["passes"] == r["passes"] + r["steps"]
    finally:
        lib.minigpt4_free(ctx)


def test_fast_verify_ex_samples_every_row_by_the_extended_rule(gpu_lib, tiny_files):
    """the one-pass form: k_sample_rows_ex over the pass's rows and k_draft_sample_finish_ex.  Every evaluated row's sample is the extended rule's pick on that row's own
    logits with draw c + 1 + r (decisions the float64 reference finds too close are left out: at most a quarter of the rows of this short text), m is the number of
    leading draft tokens the samples chose, and the conversation stands on row m."""
    lib = gpu_lib
    ctx = _spec_ctx(lib, tiny_files, parity=False)
    try:
        text = [int(lib.amd_end_chat_batch_sampled(ctx, [1], *PARAMS, with_ids=True, **SPEC_KW)[1][0]) for _ in range(12)]
        lib.amd_select_conversation(ctx, 0)
        n, judged, skipped = 0, 0, 0
        while n + 1 < len(text) and SR.EOS not in text[:n + 1]:
            draft = [t for t in text[n + 1:n + 5] if t != SR.EOS]
            c0, row0, past0 = lib.amd_sampling_info(ctx, 0)["draws"], _row(lib, ctx, 0), _n_past(lib, ctx, 0)
            r = lib.amd_verify_draft_sampled(ctx, draft, *PARAMS, want_rows=True, want_logits=True, **SPEC_KW)
            ids, rs = [int(t) for t in r["ids"]], [int(t) for t in r["row_sampled"]]
            m = len(ids) - 1
            assert ids[1:] == draft[:m] and all(rs[i] == draft[i] for i in range(m)) and (m == len(draft) or rs[m] != draft[m]) and r["next"] == rs[m]
            assert lib.amd_sampling_info(ctx, 0)["draws"] == c0 + 1 + m and _n_past(lib, ctx, 0) == past0 + 1 + m
            assert np.array_equal(_row(lib, ctx, 0), r["row_logits"][m])
            for k, (row, pick) in enumerate([(row0, ids[0])] + [(r["row_logits"][i], rs[i]) for i in range(len(draft) + 1) if rs[i] >= 0]):
                cand, vals = SR.candidates(np.asarray(row, np.float32), PARAMS[1])
                word = SR.draw_word(99, c0 + k)
                ref = CR.chain64(vals, PARAMS[0], PARAMS[2], word, **SPEC_KW)
                L = list(ref["L"])
                last = CR.last_step64(vals, L, PARAMS[0], word)
                close = len(CR.admissible_lists(vals, PARAMS[2], **SPEC_KW)) > 1 or (len(L) > 1 and np.abs(last["cum"][:-1] - last["u"]).min() < CR.MARGIN)
                if close:
                    skipped += 1
                    continue
                judged += 1
                assert int(cand[ref["pick"]]) == pick, (n, k, pick, int(cand[ref["pick"]]))
            n += 1 + m
        assert judged >= 8 and skipped <= 0.25 * (judged + skipped), (judged, skipped)
        info = lib.amd_speculation_info(ctx)
        assert info["passes"] > 0 and info["rows"] > info["passes"]          # passes of more than one row ran
    finally:
        lib.minigpt4_free(ctx)


def test_speculation_ex_refusals(gpu_lib, tiny_files):
    lib, L = gpu_lib, gpu_lib.library
    ctx = _spec_ctx(lib, tiny_files, parity=False)
    I32P = ctypes.POINTER(ctypes.c_int32)
    try:
        lib.amd_select_conversation(ctx, 0)
        lib.amd_logits(ctx)
        d, ids, one, out, st = np.array([5, 6], np.int32), np.zeros(8, np.int32), np.zeros(1, np.int32), np.zeros(8, np.int32), np.zeros(4, np.int32)
        ip = lambda x: x.ctypes.data_as(I32P)
        nan = float("nan")

        def verify(tfs_z=1.0, typical_p=1.0, min_p=0.0, temp=0.8):
            return L.minigpt4_amd_verify_draft_sampled_ex(ctx.ptr, ip(d), 2, temp, 40, 0.9, tfs_z, typical_p, min_p, ip(ids), ip(one), ip(one), None, None)

        def lookup(tfs_z=1.0, typical_p=1.0, min_p=0.0, temp=0.8):
            return L.minigpt4_amd_decode_lookup_sampled_ex(ctx.ptr, ip(d), 2, 4, 3, 1, 2, temp, 40, 0.9, tfs_z, typical_p, min_p, ip(out), ip(one), ip(st))
        before = (_n_past(lib, ctx, 0), lib.amd_sampling_info(ctx, 0), lib.amd_speculation_info(ctx))
        for f, name in ((verify, b"verify_draft_sampled_ex: "), (lookup, b"decode_lookup_sampled_ex: ")):
            for kw in (dict(tfs_z=0.0), dict(tfs_z=1.5), dict(tfs_z=nan), dict(typical_p=0.0), dict(typical_p=1.01), dict(typical_p=nan), dict(min_p=-0.1), dict(min_p=1.1),
                       dict(min_p=nan), dict(temp=0.0)):
                assert f(**kw) == 1, (name, kw)
                assert L.minigpt4_amd_last_error().startswith(name), L.minigpt4_amd_last_error()
        assert L.minigpt4_amd_verify_draft_sampled_ex(None, ip(d), 2, 0.8, 40, 0.9, 1.0, 1.0, 0.0, ip(ids), ip(one), ip(one), None, None) == 1
        assert L.minigpt4_amd_last_error().startswith(b"verify_draft_sampled_ex: no context")
        assert (_n_past(lib, ctx, 0), lib.amd_sampling_info(ctx, 0), lib.amd_speculation_info(ctx)) == before
        for call in (lib.amd_verify_draft_sampled, lambda c, dr, **kw: lib.amd_decode_lookup_sampled(c, dr, 4, **kw)):
            for kw in (dict(tfs_z=0.0), dict(typical_p=nan), dict(min_p=1.5)):
                with pytest.raises(ValueError):
                    call(None, [5, 6], **kw)                                 # the binding refuses before the library is touched
    finally:
        lib.minigpt4_free(ctx)
