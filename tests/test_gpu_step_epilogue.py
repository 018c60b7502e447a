"""The greedy step epilogues alone, against tests/greedy_ref.py (numpy): launch_argmax (k_argmax_part + k_argmax_final), k_advance, k_batch_begin / k_batch_finish,
k_gather_rows / k_seg_finish, k_draft_begin / k_draft_argmax / k_draft_finish -- the kernels that decide the greedy token and move a conversation's state at the end of
every decode step, batched step, packed prompt chunk and greedy verify pass.  One launcher call per hook call (include/minigpt4_amd_test.h).

THE RULE: the id is the lowest index holding the maximum over the row's non-NaN entries, when that maximum is above -inf; otherwise 0 (greedy_ref.first_max).

Every comparison is exact: ids and state words as integers, logits rows as uint32 bit patterns (NaN payloads and -0.0 count).  There are no tolerances.

Rows (greedy_ref.all_rows): for every length of greedy_ref.LENGTHS, one row per planted tie -- two equal maxima at every pair of places the launch geometry tells
apart (two trips of one thread, two lanes of a float4, two lanes of a wave, two waves, two workgroups of launch_argmax, the first and the last element; each with
the lower index on either side of the compare: tests/test_cpu_step_epilogue.py checks that cover) -- and the special rows: a single peak (at n = 32001: in the last
scalar trip only), all equal, -0.0 against +0.0 both ways, all -inf, all NaN, NaN and -inf only, NaN at index 0 / round the peak / sprinkled."""
import numpy as np
import pytest

import greedy_ref as G

pytestmark = pytest.mark.gpu

_ROWS = {}


def _rows(n):
    """(labels, rows [k][n], expected ids) of length n: built once, shared, never written to."""
    if n not in _ROWS:
        r = G.all_rows(n)
        x = np.stack([t[1] for t in r])
        x.setflags(write=False)
        _ROWS[n] = ([t[0] for t in r], x, np.array([t[2] for t in r], np.int32))
    return _ROWS[n]


def _finish_ids(lib, form, x):
    """The ids k_batch_finish (form 0) / k_seg_finish (form 1) give the rows of x, 64 rows a launch, through a reversed row-to-slot map; the copies are checked on the way."""
    ids = []
    for a in range(0, len(x), 64):
        blk = x[a:a + 64]
        rows, n = blk.shape
        st = G.start_state(rows, n, a)
        sl = np.arange(rows - 1, -1, -1, dtype=np.int32)
        d = sl if form == 0 else np.stack([sl, 7000 + np.arange(rows, dtype=np.int32)], 1)
        got = lib.amd_test_step_finish(form, blk, d, st["n_past"], st["argmax"], st["feed"], st["slot_logits"])
        assert np.array_equal(got["argmax"][sl], got["feed"][sl])
        assert np.array_equal(G.bits(got["slot_logits"][sl]), G.bits(blk)) and np.array_equal(G.bits(got["slot_logits"][rows]), G.bits(st["slot_logits"][rows]))
        assert got["argmax"][rows] == st["argmax"][rows] and got["feed"][rows] == st["feed"][rows] and got["n_past"][rows] == st["n_past"][rows]
        want_pos = st["n_past"][:rows] + 1 if form == 0 else (7000 + np.arange(rows, dtype=np.int32))[::-1]
        assert np.array_equal(got["n_past"][:rows], want_pos)
        ids += got["argmax"][sl].tolist()
    return np.array(ids, np.int32)


def _draft_ids(lib, x):
    """The ids k_draft_argmax gives the rows of x, 8 rows a launch; the words behind R keep the fill."""
    ids = []
    for a in range(0, len(x), 8):
        blk = x[a:a + 8]
        R, n = blk.shape
        st = G.start_state(3, n, a)
        got = lib.amd_test_draft_finish(blk, np.full(R, -5, np.int32), 1, st["n_past"], st["argmax"], st["feed"], st["slot_logits"])
        assert got["m"] == 0 and (got["res"][1 + R:] == -1).all()
        ids += got["res"][1:1 + R].tolist()
    return np.array(ids, np.int32)


def _report(labels, got, want, n, what):
    bad = [(labels[i], int(got[i]), int(want[i])) for i in np.flatnonzero(got != want)]
    assert not bad, f"{what}, n = {n}: (row, got, want) {bad[:12]} ({len(bad)} of {len(want)} rows)"


@pytest.mark.parametrize("n", G.LENGTHS)
def test_launch_argmax_first_maximum(gpu_lib, n):
    labels, x, want = _rows(n)
    got = np.empty(len(x), np.int32)
    for k in range(len(x)):
        got[k], pv, pi = gpu_lib.amd_test_argmax(x[k])
        # the 64 workgroups' partials: workgroup g saw the elements i with (i // 256) % 64 == g; none: value -inf, id 0x7FFFFFFF
        for g in sorted({0, 1, 63, (want[k] // 256) % 64}):
            mine = np.flatnonzero((np.arange(n) // 256) % 64 == g)
            sub = x[k][mine]
            ok = len(mine) > 0 and bool((~np.isnan(sub)).any()) and bool(np.nanmax(sub) > -np.inf)
            if ok:
                assert pi[g] == mine[G.first_max(sub)] and G.bits(pv[g:g + 1])[0] in set(G.bits(sub[sub == np.nanmax(sub)]).tolist()), (n, labels[k], g)
            else:
                assert pi[g] == 0x7FFFFFFF and pv[g] == -np.inf, (n, labels[k], g)
    _report(labels, got, want, n, "launch_argmax")


@pytest.mark.parametrize("form", [0, 1], ids=["batch_finish", "seg_finish"])
@pytest.mark.parametrize("n", G.LENGTHS)
def test_finish_kernels_first_maximum(gpu_lib, n, form):
    labels, x, want = _rows(n)
    _report(labels, _finish_ids(gpu_lib, form, x), want, n, ("k_batch_finish", "k_seg_finish")[form])


@pytest.mark.parametrize("n", G.LENGTHS)
def test_draft_argmax_first_maximum(gpu_lib, n):
    labels, x, want = _rows(n)
    _report(labels, _draft_ids(gpu_lib, x), want, n, "k_draft_argmax")


@pytest.mark.parametrize("n", G.LENGTHS)
def test_family_agrees_on_one_id(gpu_lib, n):
    """launch_argmax, k_batch_finish, k_seg_finish, k_draft_argmax, k_logprob_rows' greedy id and first_max: one number on every NaN-free row with a maximum above -inf."""
    labels, x, want = _rows(n)
    keep = np.array([G.agrees_everywhere(r) for r in x])
    assert keep.sum() >= 3 and (n < 2 or keep.sum() >= len(G.tie_pairs(n)) + 6)
    labels, x, want = [l for l, k in zip(labels, keep) if k], x[keep], want[keep]
    six = dict(first_max=np.array([G.first_max(r) for r in x], np.int32),
               launch_argmax=np.array([gpu_lib.amd_test_argmax(r)[0] for r in x], np.int32),
               k_batch_finish=_finish_ids(gpu_lib, 0, x), k_seg_finish=_finish_ids(gpu_lib, 1, x), k_draft_argmax=_draft_ids(gpu_lib, x),
               k_logprob_rows=np.asarray(gpu_lib.amd_test_logprob_rows(x, np.full(len(x), -1, np.int32))[1], np.int32))
    for name, got in six.items():
        _report(labels, got, want, n, name)


# ---- state ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _state_rows(rows, n):
    """rows logits rows of length n: ties and specials of that length, evenly picked from the list (so their ids differ), then seeded draws with one peak each."""
    labels, x, want = _rows(n)
    take = [x[k] for k in np.linspace(0, len(x) - 1, min(rows, len(x))).astype(int)]
    take += [G.planted_row(n, 5000 + r, ((37 * r + 11) % n,)) for r in range(rows - len(take))]
    return np.stack(take)


@pytest.mark.parametrize("n", [32000, 32001, 260, 257])
@pytest.mark.parametrize("rows", [1, 2, 5, 64])
@pytest.mark.parametrize("form", [0, 1], ids=["batch_finish", "seg_finish"])
def test_finish_state(gpu_lib, form, rows, n):
    n_slot = rows + 3
    lg = _state_rows(rows, n)
    for name, sl in G.slot_maps(rows, n_slot, n).items():
        st = G.start_state(n_slot, n, rows)
        d = sl if form == 0 else np.stack([sl, (900 + 13 * np.arange(rows)).astype(np.int32)], 1)
        got = gpu_lib.amd_test_step_finish(form, lg, d, st["n_past"], st["argmax"], st["feed"], st["slot_logits"])
        ref = G.finish_ref(form, lg, d, st)
        for k in ("n_past", "argmax", "feed"):
            assert np.array_equal(got[k], ref[k]), (name, k, got[k].tolist(), ref[k].tolist())
        same = (G.bits(got["slot_logits"]) == G.bits(ref["slot_logits"])).all(axis=1)
        assert same.all(), (name, "slot_logits rows that differ", np.flatnonzero(~same).tolist(), "row -> slot", sl.tolist())
        untouched = sorted(set(range(n_slot + 1)) - set(sl.tolist()))                        # the three free slots and the guard: exactly as given
        assert np.array_equal(G.bits(got["slot_logits"][untouched]), G.bits(st["slot_logits"][untouched]))
        for k in ("n_past", "argmax", "feed"):
            assert np.array_equal(got[k][untouched], st[k][untouched]), (name, k)


def _draft_case(lib, lg, ids, tok, n_vocab):
    st = G.start_state(3, n_vocab, len(lg))
    for slot in (1, 2):
        got = lib.amd_test_draft_finish(lg, tok, slot, st["n_past"], st["argmax"], st["feed"], st["slot_logits"])
        ref = G.draft_finish_ref(lg, tok, slot, st)
        assert got["m"] == ref["m"], (tok.tolist(), ids, got["res"].tolist())
        assert np.array_equal(got["res"], ref["res"]), (got["res"].tolist(), ref["res"].tolist())
        for k in ("n_past", "argmax", "feed"):
            assert np.array_equal(got[k], ref[k]), (k, slot, got[k].tolist(), ref[k].tolist())
        assert np.array_equal(G.bits(got["slot_logits"]), G.bits(ref["slot_logits"])), slot
        m = ref["m"]
        assert got["argmax"][slot] == got["feed"][slot] == got["res"][1 + m] and got["n_past"][slot] == st["n_past"][slot] + 1 + m
        assert np.array_equal(G.bits(got["slot_logits"][slot]), G.bits(lg[m]))
    return ref["m"]


@pytest.mark.parametrize("n", [32000, 32001, 1025])
@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_draft_finish(gpu_lib, R, n):
    lg = _state_rows(R, n)                                                    # ties, single peaks, an all-equal row, ... : R of them
    ids = [G.first_max(r) for r in lg]
    seen = set()
    for m in range(R):                                                       # m = 0, every middle value, R - 1
        seen.add(_draft_case(gpu_lib, lg, ids, G.draft_toks(ids, m), n))
    assert seen == set(range(R))
    for m in range(R - 2):                                                   # a mismatch followed by later matches: they do not count
        tok = G.draft_toks(ids, m, later_match=True)
        assert _draft_case(gpu_lib, lg, ids, tok, n) == m


# ---- bookkeeping words and the gather ----------------------------------------------------------------------------------------------------------------------------------
def _words(n_slot, seed):
    st = G.start_state(n_slot, 1, seed)
    return st["n_past"], st["argmax"], st["feed"]


@pytest.mark.parametrize("with_tok0", [True, False])
@pytest.mark.parametrize("n", [1, 37])
def test_advance(gpu_lib, n, with_tok0):
    for n_slot, slot in ((1, 0), (4, 2), (4, 3)):
        a, b, c = _words(n_slot, n)
        got = gpu_lib.amd_test_step_words(0, [slot], a, b, c, n=n, with_tok0=with_tok0)
        wa, wc = a.copy(), c.copy()
        wa[slot] += n
        if with_tok0:
            wc[slot] = b[slot]
        assert np.array_equal(got["n_past"], wa) and np.array_equal(got["argmax"], b) and np.array_equal(got["feed"], wc), (n_slot, slot)


@pytest.mark.parametrize("B", [1, 5, 64])
def test_batch_begin(gpu_lib, B):
    n_slot = B + 3
    for name, sl in G.slot_maps(B, n_slot, 3).items():
        a, b, c = _words(n_slot, B)
        pos = (40 + 7 * np.arange(B)).astype(np.int32)
        got = gpu_lib.amd_test_step_words(1, sl, a, b, c, row_pos=pos)
        wa = a.copy()
        wa[sl] = pos
        assert np.array_equal(got["n_past"], wa) and np.array_equal(got["argmax"], b) and np.array_equal(got["feed"], c), name
    if B > 1:                                                                # fewer rows than the arrays hold: the rows behind B are not applied
        a, b, c = _words(n_slot, B)
        got = gpu_lib.amd_test_step_words(1, sl, a, b, c, row_pos=pos, n=B - 1)
        wa = a.copy()
        wa[sl[:B - 1]] = pos[:B - 1]
        assert np.array_equal(got["n_past"], wa)


def test_draft_begin(gpu_lib):
    for n_slot, slot in ((1, 0), (3, 1), (3, 2)):
        a, b, c = _words(n_slot, slot)
        got = gpu_lib.amd_test_step_words(2, [slot], a, b, c, row_pos=[123])
        wa = a.copy()
        wa[slot] = 123
        assert np.array_equal(got["n_past"], wa) and np.array_equal(got["argmax"], b) and np.array_equal(got["feed"], c)


@pytest.mark.parametrize("E", [1, 255, 256, 257, 5120])
def test_gather_rows(gpu_lib, E):
    n_src = 9
    src = np.random.default_rng(E).standard_normal((n_src, E)).astype(np.float32)
    w = src.view(np.uint32)
    w[:, ::5] = G.nan_with_payload(n_src * len(range(0, E, 5))).view(np.uint32).reshape(n_src, -1)      # NaN bit patterns, distinct ones
    w[3, E // 2] = 0x80000000                                                                           # -0.0
    for idx in ([4], [0], [8], [8, 7, 6, 5, 4, 3, 2], [2, 2, 5, 2, 0, 8, 8]):                            # n of 1 and 7; descending; repeated
        got = gpu_lib.amd_test_gather_rows(src, idx).view(np.uint32)
        assert got.shape == (len(idx) + 1, E)
        assert np.array_equal(got[:-1], w[idx]), idx
        assert (got[-1] == G.FILL32).all(), idx
