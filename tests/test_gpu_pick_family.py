"""The three device picks walk ONE transformed row (pick_row.hpp): k_pen_pick, k_constrain_pick and k_sample_rows mark the same table ids, sweep the same unmarked ids and
value the table ids through the same function.  What each kernel computes is held to numpy elsewhere (test_gpu_penalties, test_gpu_constraint, test_gpu_device_sampling);
here the kernels are held to EACH OTHER, through the existing hooks, on the same inputs:

  1. every id allowed: the constrained pick is the penalised pick, never stuck;
  2. top_k = 1: the sampled pick is the constrained pick under the same bitmap (no bitmap: under the all-ones one), for two seeds and two draw counts -- one candidate,
     one kept, ids[0] = the pick, probability exactly 1.0f, not stuck;
  3. nothing allowed: CONSTRAINT_EOS | CONSTRAIN_STUCK from the constrained pick; pick = CONSTRAINT_EOS, stuck = 1, no candidate, every id -1 from the sampled one;
  4. only table ids allowed (the row sweep contributes nothing): 1 and 2 still hold, and the pick is the numpy reference's (constraint_ref.pick_ref).

Rows: a seeded normal draw capped below the planted maximum, which sits at three ids -- the lowest of them a table id wherever the row has a table, and there with a
bias of +0.0 where the scenario has a bias, so that the tie survives the transformation and "the lower id wins" has to hold ACROSS the table loop and the row sweep.
No element is +-0, before or after the transformation (asserted): the greedy combine treats -0 and +0 as equal, the sampling key need not.
Tables: 0, 1 and min(PEN_TABLE_MAX, 300) entries (the last: a thread takes more than one entry), capped at n_vocab distinct ids and -- bias alone -- at the 256 a bias
list holds; repetition penalty on / off x frequency and presence on / off, each with and without a bias."""
import numpy as np
import pytest

import constraint_ref as R
from test_cpu_penalties import make_row
from test_gpu_penalties import _f32_word

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 31, 31), (3, 33, 40), (2, 100, 101), (3, 513, 521), (2, 32001, 32001)]   # (rows, n_vocab, ld)
PEN_TABLE_MAX, PEN_BIAS_MAX = 1281, 256
TABLES = [0, 1, min(PEN_TABLE_MAX, 300)]
PEAK = np.float32(9.0)
SEEDS, DRAWS = (0x1234567, 0xFEDCBA9876543210), (0, 5)
TEMP, TOP_P = 0.7, 0.9
STUCK = 1 << 30
N_CTX = 4096


def _bitmap(n_vocab, ids):
    ok = np.zeros(R.index_words(n_vocab) * 32, bool)
    ok[list(ids)] = True
    return np.packbits(ok, bitorder="little").view(np.uint32)


def _scenario(lib, n_vocab, seed, n_table, rep, alpha, bias_on):
    """One row as a conversation presents it: dict(x, history, kw, bias, tab [n][4], words [8] without the buffer row and the offset filled in, t = the transformed row)."""
    rng = np.random.default_rng(seed)
    x = np.minimum(make_row(n_vocab, seed), np.float32(8.0))
    peaks = sorted({n_vocab // 5, n_vocab // 2, n_vocab - 1})
    x[peaks] = PEAK
    assert not (x == 0).any()
    pen_on = rep or alpha
    n = min(n_table, n_vocab) if (pen_on or bias_on) else 0
    if not pen_on:
        n = min(n, PEN_BIAS_MAX)
    ids = [peaks[0]] + [int(i) for i in rng.permutation(n_vocab) if i != peaks[0]]          # the lowest peak first: it is in every table
    ids = ids[:n]
    history, bias, kw = [], {}, {}
    if pen_on:
        n_hist = n if not bias_on else max(1, (2 * n) // 3)                                # with a bias: a third of the entries are bias-only
        history = [i for i in ids[:n_hist] for _ in range(1 + i % 3)]                       # counts 1 .. 3
        assert len(history) <= 1024                                                         # the window holds them all
        kw = dict(repeat_last_n=-1, repeat_penalty=1.3 if rep else 1.0, alpha_frequency=0.25 if alpha else 0.0, alpha_presence=0.5 if alpha else 0.0)
        if bias_on:
            for j, i in enumerate(ids[n_hist:] + ids[:n_hist:4]):
                bias[i] = float(np.float32(((j % 7) - 3) * 0.375 + 0.125))
    elif bias_on:
        for j, i in enumerate(ids):
            bias[i] = float(np.float32(((j % 7) - 3) * 0.375 + 0.125))
    if bias_on and n and not pen_on:
        bias[peaks[0]] = 0.0                                                                # the planted tie survives: value + (+0.0)
    t, tab, flags = lib.amd_test_penalise_host(x, history, N_CTX, bias=bias, **kw)
    assert len(tab) == n, (len(tab), n)
    assert not (t == 0).any()
    p = dict(repeat_penalty=1.0, alpha_presence=0.0, alpha_frequency=0.0)
    p.update({k: v for k, v in kw.items() if k in p})
    words = [0, 0, len(tab), flags, _f32_word(p["repeat_penalty"]), _f32_word(p["alpha_frequency"]), _f32_word(p["alpha_presence"]), 0]
    return dict(x=x, history=history, kw=kw, bias=bias, tab=tab, words=words, t=t, peaks=peaks)


_CASES = {}


def _launches(lib, shape):
    """Every scenario of a shape, `rows` per launch: [dict(buf, rows [rows][8], table [m][4], scen [rows])], built once."""
    if shape in _CASES:
        return _CASES[shape]
    rows, n_vocab, ld = shape
    combos = [(n, rep, alpha, b) for n in TABLES for rep in (0, 1) for alpha in (0, 1) for b in (0, 1)]
    combos = [c for c in combos if (c[0] > 0) == bool(c[1] or c[2] or c[3])]             # an empty table is the identity and nothing else is
    out = []
    for first in range(0, len(combos), rows):
        buf = np.full((rows, ld), 1e9, np.float32)                                         # the stride's padding would win every pick if it were read
        rw, table, scen = [], [], []
        for r in range(rows):
            n, rep, alpha, b = combos[(first + r) % len(combos)]
            s = _scenario(lib, n_vocab, 7000 * n_vocab + first + r, n, rep, alpha, b)
            buf[r, :n_vocab] = s["x"]
            rw.append([r, len(table)] + s["words"][2:])
            table += s["tab"].tolist()
            scen.append(s)
        out.append(dict(buf=buf, rows=np.array(rw, np.int32), table=np.array(table, np.int32).reshape(-1, 4), scen=scen))
    _CASES[shape] = out
    return out


def _sample(lib, L, n_vocab, seed, draws, bitmaps, bitmap_of_row):
    n = len(L["rows"])
    return lib.amd_test_sample_rows(L["buf"], n_vocab, L["rows"], L["table"], [[TEMP, TOP_P]] * n, [1] * n, [[seed, draws + r] for r in range(n)],
                                    bitmaps=bitmaps, bitmap_of_row=bitmap_of_row)


def _assert_one_candidate(o, want, what):
    n = len(want)
    assert o["pick"].tolist() == list(want), (what, o["pick"].tolist(), list(want))
    assert o["n_cand"].tolist() == [1] * n and o["kept"].tolist() == [1] * n, (what, o["n_cand"], o["kept"])
    assert o["ids"][:, 0].tolist() == list(want) and (o["ids"][:, 1:] == -1).all(), what
    assert (o["p"][:, 0].view(np.uint32) == np.float32(1.0).view(np.uint32)).all(), (what, o["p"][:, 0])
    assert o["stuck"].tolist() == [0] * n, what


@pytest.mark.parametrize("rows,n_vocab,ld", SHAPES)
def test_every_id_allowed_the_constrained_pick_is_the_penalised_pick(gpu_lib, rows, n_vocab, ld):
    ones = _bitmap(n_vocab, range(n_vocab))[None, :]
    tied = 0
    for L in _launches(gpu_lib, (rows, n_vocab, ld)):
        pen, _, _ = gpu_lib.amd_test_pen_pick(L["buf"], n_vocab, L["rows"], L["table"])
        con, stuck, _ = gpu_lib.amd_test_constrain_pick(L["buf"], n_vocab, L["rows"], L["table"], ones, [0] * rows)
        assert con.tolist() == pen.tolist() and not stuck.any(), (con, pen, stuck)
        for r, s in enumerate(L["scen"]):                                                  # the scenarios are what the docstring says: the lower id of a tie wins
            top = np.flatnonzero(s["t"] == s["t"].max())
            assert int(pen[r]) == int(top[0])
            tied += len(top) > 1
    assert tied >= 1 or n_vocab < 3                                                        # (fewer than three ids: the planted ids coincide)


@pytest.mark.parametrize("rows,n_vocab,ld", SHAPES)
def test_one_candidate_the_sampled_pick_is_the_constrained_pick(gpu_lib, rows, n_vocab, ld):
    rng = np.random.default_rng(31 * n_vocab + rows)
    ones = _bitmap(n_vocab, range(n_vocab))
    for L in _launches(gpu_lib, (rows, n_vocab, ld)):
        some = []
        for r in range(rows):
            ids = set(np.flatnonzero(rng.random(n_vocab) < 0.5).tolist()) | {int(rng.integers(n_vocab))}   # at least one bit
            some.append(_bitmap(n_vocab, ids))
        bitmaps = np.array([ones] + some)
        for name, of_row, of_row_con in (("all ones", [0] * rows, [0] * rows), ("null", None, [0] * rows), ("random", list(range(1, rows + 1)), list(range(1, rows + 1)))):
            con, stuck, _ = gpu_lib.amd_test_constrain_pick(L["buf"], n_vocab, L["rows"], L["table"], bitmaps, of_row_con)
            assert not stuck.any()
            for seed in SEEDS:
                for draws in DRAWS:
                    _assert_one_candidate(_sample(gpu_lib, L, n_vocab, seed, draws, bitmaps, of_row), con.tolist(), (name, seed, draws))


@pytest.mark.parametrize("rows,n_vocab,ld", SHAPES)
def test_nothing_allowed(gpu_lib, rows, n_vocab, ld):
    zeros = np.zeros((1, R.index_words(n_vocab)), np.uint32)
    for L in _launches(gpu_lib, (rows, n_vocab, ld)):
        con, stuck, _ = gpu_lib.amd_test_constrain_pick(L["buf"], n_vocab, L["rows"], L["table"], zeros, [0] * rows)
        assert con.tolist() == [R.EOS] * rows and stuck.all()
        o = _sample(gpu_lib, L, n_vocab, SEEDS[0], DRAWS[0], zeros, [0] * rows)
        assert o["pick"].tolist() == [R.EOS] * rows and o["stuck"].tolist() == [1] * rows
        assert o["n_cand"].tolist() == [0] * rows and o["kept"].tolist() == [0] * rows and (o["ids"] == -1).all()


@pytest.mark.parametrize("rows,n_vocab,ld", SHAPES)
def test_only_table_ids_allowed(gpu_lib, rows, n_vocab, ld):
    checked = 0
    for L in _launches(gpu_lib, (rows, n_vocab, ld)):
        if any(len(s["tab"]) == 0 for s in L["scen"]):                                     # (an empty table allows nothing: test_nothing_allowed)
            continue
        bitmaps = np.array([_bitmap(n_vocab, s["tab"][:, 0].tolist()) for s in L["scen"]])
        of_row = list(range(rows))
        con, stuck, _ = gpu_lib.amd_test_constrain_pick(L["buf"], n_vocab, L["rows"], L["table"], bitmaps, of_row)
        want = [R.pick_ref(s["x"], bitmaps[r], history=s["history"], n_ctx=N_CTX, bias=s["bias"], **s["kw"]) for r, s in enumerate(L["scen"])]
        assert [(int(i), bool(k)) for i, k in zip(con, stuck)] == want, (con, stuck, want)
        for seed in SEEDS:
            for draws in DRAWS:
                _assert_one_candidate(_sample(gpu_lib, L, n_vocab, seed, draws, bitmaps, of_row), con.tolist(), ("table ids", seed, draws))
        checked += 1
    assert checked >= 1
