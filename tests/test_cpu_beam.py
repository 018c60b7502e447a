"""Beam search without a device: the rule's host function and the engine's book-keeping (minigpt4_amd_test_beam_select_host: csrc/beam.hpp + csrc/beam_host.hpp) against
the NumPy float32 restatement tests/beam_ref.py -- every step's result block word for word, the hypotheses, their order, their scores bit for bit, the statistics -- and
the refusals of the entry point and of the binding, which need no GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import beam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P, F32P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
HOOKS = ("minigpt4_amd_test_beam_select_host", "minigpt4_amd_test_beam_select", "minigpt4_amd_test_kv_permute")


def make_cands(rng, T, W, grid=None, eos_at=(), vocab=500):
    """ids / lp [T][W][2 W]: distinct ids per row (never EOS unless placed), log-probabilities descending along a row; grid: round them to multiples of it (ties).
    eos_at: (step, beam, column) places where the id is EOS."""
    C = 2 * W
    ids = np.zeros((T, W, C), np.int32)
    lp = np.zeros((T, W, C), np.float32)
    for t in range(T):
        for i in range(W):
            ids[t, i] = rng.choice(np.arange(3, vocab), C, replace=False)
            v = -np.sort(rng.exponential(1.5, C)).astype(np.float32)
            if grid:
                v = (np.round(v / grid) * grid).astype(np.float32)
            lp[t, i] = v
    for t, i, c in eos_at:
        ids[t, i, c] = R.EOS
    return ids, lp


def check(lib, ids, lp, lpen, n_best=None, position=0):
    got = lib.amd_test_beam_select_host(ids, lp, length_penalty=lpen, n_best=n_best, position=position)
    hyps, stats, s = R.search_given(ids, lp, lpen, n_best, position)
    W = ids.shape[1]
    assert list(got["stats"]) == stats
    assert len(got["steps"]) == s.steps
    for t, d in enumerate(s.log):
        assert np.array_equal(got["steps"][t], R.pack_step(W, d)), t
    assert len(got["hyps"]) == len(hyps)
    for (a, sa), (b, sb) in zip(got["hyps"], hyps):
        assert np.array_equal(a, b)
        assert np.float32(sa).tobytes() == np.float32(sb).tobytes()
    return got, s


@pytest.mark.parametrize("W", [2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("lpen", [0.0, 1.0, 0.7])
def test_random_searches_equal_the_restatement(lib, W, lpen):
    rng = np.random.default_rng(100 * W + int(10 * lpen))
    for _ in range(4):
        ids, lp = make_cands(rng, 6, W)
        got, s = check(lib, ids, lp, lpen, position=5)
        assert s.steps == 6 and not s.full                       # no EOS anywhere: ends on max_tokens, every hypothesis unfinished and 6 tokens long
        assert all(len(h[0]) == 6 for h in got["hyps"]) and len(got["hyps"]) == W


@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_equal_scores_across_and_inside_beams(lib, W):
    rng = np.random.default_rng(7 + W)
    for grid in (0.5, 2.0, 100.0):                               # 100: every log-probability rounds to 0 or -0 -- all candidates tie, beam then column decide
        ids, lp = make_cands(rng, 5, W, grid=grid)
        lp[lp == 0] = np.where(rng.random(int((lp == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))   # -0 and +0 must tie
        _, s = check(lib, ids, lp, 1.0)
        if grid == 100.0:
            assert s.log[1]["parent"] == [0] * W                 # all equal: beam 0's columns 0 .. W - 1
            assert s.log[1]["tok"] == [int(x) for x in ids[1, 0, :W]]


def test_eos_below_w_finishes_and_above_w_is_skipped(lib):
    W = 3
    rng = np.random.default_rng(3)
    ids, lp = make_cands(rng, 4, W, eos_at=[(1, 0, 0)])          # step 1: beam 0's best token is EOS
    lp[1, 0, 0] = -0.01
    _, s = check(lib, ids, lp, 1.0)
    assert len(s.log[1]["fin"]) == 1 and s.finished == 1
    # the same EOS made unlikely: it ranks at W or beyond, finishes nothing and is walked past
    ids2, lp2 = ids.copy(), lp.copy()
    lp2[1, 0] = np.sort(lp2[1, 0])[::-1]
    ids2[1, 0, 0], ids2[1, 0, 5] = ids2[1, 0, 5], R.EOS
    lp2[1, 0, 5] = -50.0
    lp2[1, 0] = np.sort(lp2[1, 0])[::-1]
    _, s2 = check(lib, ids2, lp2, 1.0)
    assert s2.finished == 0 and all(R.EOS not in d["tok"] for d in s2.log)


def test_eos_skipped_inside_the_walk(lib):
    """An EOS at a rank >= W that the walk still has to pass: the first W ranks hold a finished EOS, so filling W beams reaches rank W + 1."""
    W = 2
    ids = np.array([[[10, 11, 12, 13], [0, 0, 0, 0]], [[2, 20, 21, 22], [23, 2, 24, 25]]], np.int32)
    lp = np.array([[[-0.1, -0.2, -3, -4], [0, 0, 0, 0]], [[-0.1, -5, -6, -7], [-0.2, -0.3, -8, -9]]], np.float32)
    ids[0, 1] = [30, 31, 32, 33]
    _, s = check(lib, ids, lp, 0.0)
    d = s.log[1]
    assert len(d["fin"]) == 1 and d["fin"][0][0] == 0           # rank 0: beam 0's EOS finishes; rank 2: beam 1's EOS is skipped
    assert d["tok"] == [23, 20] and d["parent"] == [1, 0]


@pytest.mark.parametrize("W", [2, 4, 8])
def test_eos_in_every_beam_at_once_ends_the_search(lib, W):
    rng = np.random.default_rng(50 + W)
    ids, lp = make_cands(rng, 5, W, eos_at=[(2, i, 0) for i in range(W)])
    lp[2, :, 0] = -0.001                                         # every beam's EOS sits in the first W ranks
    lp[2, :, 1:] -= 5.0
    got, s = check(lib, ids, lp, 0.7)
    assert s.full and s.steps == 3 and s.finished == W           # termination by W finished, in the step that brought them
    assert all(h[0][-1] == R.EOS and len(h[0]) == 3 for h in got["hyps"])


def test_first_step_takes_beam_zero_only(lib):
    W = 4
    rng = np.random.default_rng(9)
    ids, lp = make_cands(rng, 1, W)
    lp[0, 1:] = 0.0                                              # dead beams with better numbers: ignored
    got, s = check(lib, ids, lp, 1.0)
    assert s.log[0]["parent"] == [0] * W and s.log[0]["tok"] == [int(x) for x in ids[0, 0, :W]]
    assert list(got["stats"]) == [1, 0, 0, 0]                    # parents differ from the identity, but no row lies between `common` and the position yet


def test_finished_list_overflow_keeps_the_best_under_the_tie_rule(lib):
    """W = 3, two hypotheses finished in step 1 and two more in step 2: four candidates for three places.  With length_penalty 0 and equal raw scores the earlier creation
    wins, so the LAST created one is dropped."""
    W = 3
    rng = np.random.default_rng(11)
    ids, lp = make_cands(rng, 4, W)
    lp[:] = -4.0
    lp[0, 0, :3] = [-1.0, -1.0, -1.0]
    ids[1, 0, 0] = ids[1, 1, 0] = R.EOS                          # step 1: beams 0 and 1 finish at -1 + -1 = -2
    lp[1, :, 0] = -1.0
    lp[1, :, 1] = -1.0
    ids[2, 0, 0] = ids[2, 1, 0] = R.EOS                          # step 2: two more at -1 + -1 + 0 = -2
    lp[2, :, 0] = 0.0
    lp[2, :, 1] = 0.0
    got, s = check(lib, ids, lp, 0.0)
    assert s.finished == 4 and s.full and s.steps == 3 and len(got["hyps"]) == 3
    assert [len(h[0]) for h in got["hyps"]] == [2, 2, 3]          # equal scores: creation order; the fourth is dropped
    got1, _ = check(lib, ids, lp, 1.0)                           # normalised: -2 / 2 against -2 / 3 -- the later, longer ones lead now
    assert [len(h[0]) for h in got1["hyps"]] == [3, 3, 2]
    check(lib, ids, lp, 0.7, n_best=1)


def test_finished_rank_before_unfinished_at_equal_scores(lib):
    W = 2
    ids = np.array([[[10, 11, 12, 13], [14, 15, 16, 17]], [[2, 20, 21, 22], [23, 24, 25, 26]]], np.int32)
    lp = np.array([[[-1, -1, -5, -6], [0, 0, 0, 0]], [[-1, -1, -7, -8], [-1, -1, -7, -8]]], np.float32)
    got, s = check(lib, ids, lp, 0.0)
    assert s.finished == 1 and not s.full
    assert [float(h[1]) for h in got["hyps"]] == [-2.0, -2.0] and got["hyps"][0][0][-1] == R.EOS
    assert len(R.search_given(ids, lp, 0.0)[0]) == 2 and len(s.done) == 3


def test_rows_moved_follow_the_common_rule(lib):
    """Parents all equal -> the rows below that step's position are shared from then on; a later permutation moves only the rows above."""
    W = 2
    rng = np.random.default_rng(21)
    ids, lp = make_cands(rng, 5, W)
    lp[:] = -9.0
    lp[0, 0, :2] = [-1, -2]
    lp[1, 0, :2] = [-1, -1.5]                                    # step 1: both from beam 0: 1 conversation x 1 row (the row step 0 wrote), then common = position + 1
    lp[2, 0, 0], lp[2, 1, 0] = -3, -1                            # step 2: parents [1, 0], a swap: 2 conversations x 1 row
    lp[3, 0, 0], lp[3, 1, 0] = -1, -1                            # step 3: identity
    lp[4, 1, :2] = [-1, -1]                                      # step 4: both from beam 1: 1 conversation x 3 rows
    got, s = check(lib, ids, lp, 1.0, position=7)
    assert [d["parent"] for d in s.log] == [[0, 0], [0, 0], [1, 0], [0, 1], [1, 1]]
    assert list(got["stats"]) == [5, 3, 1 * 1 + 2 * 1 + 1 * 3, 0]


def test_hooks_and_entry_point_are_where_they_belong(lib):
    def exported(so):
        return set(re.findall(r" T (minigpt4_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)))

    def declared(header):
        return set(re.findall(r"MINIGPT4_API[^;]*?\b(minigpt4_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))
    product, test = exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so")), exported(os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4_test.so"))
    assert "minigpt4_amd_beam_search" in product and "minigpt4_amd_beam_search" in declared("minigpt4_amd.h")
    for h in HOOKS:
        assert h in test and h not in product and h in declared("minigpt4_amd_test.h") and h not in declared("minigpt4_amd.h")


def test_refusals_without_a_device(lib):
    L = lib.library
    sl = np.array([0, 1], np.int32)
    tok, ln, sc, n, st = np.zeros((2, 5), np.int32), np.zeros(2, np.int32), np.zeros(2, np.float32), np.zeros(1, np.int32), np.zeros(4, np.int32)
    ip, fp = (lambda a: a.ctypes.data_as(I32P)), (lambda a: a.ctypes.data_as(F32P))
    assert L.minigpt4_amd_beam_search(None, ip(sl), 2, 4, 1.0, 2, ip(tok), ip(ln), fp(sc), ip(n), ip(st)) == 1
    assert L.minigpt4_amd_last_error().startswith(b"beam_search: no context")
    with pytest.raises(RuntimeError, match="beam_search"):
        lib.amd_beam_search(None, [0, 1], 4)
    for bad in (dict(slots=[0], max_tokens=4), dict(slots=list(range(9)), max_tokens=4), dict(slots=[0, 1], max_tokens=0), dict(slots=[0, 1], max_tokens=4, n_best=3),
                dict(slots=[0, 1], max_tokens=4, n_best=0), dict(slots=[0, 1], max_tokens=4, length_penalty=float("inf")), dict(slots=[0, 1], max_tokens=4, length_penalty=float("nan"))):
        with pytest.raises(ValueError, match="beam_search"):
            lib.amd_beam_search(None, **bad)                     # refused by the binding before the library is touched
    # the host hook: bad arguments
    ids, lp = make_cands(np.random.default_rng(1), 2, 2)
    H = L.minigpt4_amd_test_beam_select_host
    args = lambda **kw: [kw.get("W", 2), kw.get("T", 2), kw.get("ids", ip(ids)), kw.get("lp", fp(lp)), None, 0, 2, 0, kw.get("pen", 1.0), kw.get("nb", 2), None,
                         kw.get("tok", ip(tok)), ip(ln), fp(sc), ip(n), ip(st)]
    assert H(*args()) == 0
    for kw in (dict(W=1), dict(W=9), dict(T=0), dict(ids=None), dict(lp=None), dict(nb=0), dict(nb=3), dict(tok=None), dict(pen=float("nan"))):
        assert H(*args(**kw)) == 1, kw
    two_eos = ids.copy()
    two_eos[0, 0, :3] = 2                                        # the first step cannot fill two beams from one token that is not EOS
    assert H(*args(ids=ip(two_eos))) == 1
    # the kernel hooks refuse before they look for a device
    P = L.minigpt4_amd_test_kv_permute
    k = np.zeros((3, 1, 4, 8), np.uint16)
    kp = k.ctypes.data_as(ctypes.c_void_p)
    call = lambda slots=(0, 1), parent=(1, 0), r0=0, r1=4, n=None, e=8: P(3, 1, 4, e, ip(np.array(slots, np.int32)), len(slots) if n is None else n,
                                                                          ip(np.array(parent, np.int32)), r0, r1, kp, kp, None)
    for kw in (dict(slots=(0, 0)), dict(slots=(0, 3)), dict(slots=(0, -1)), dict(parent=(2, 0)), dict(parent=(-1, 0)), dict(r0=-1), dict(r0=3, r1=2), dict(r1=5), dict(n=1),
               dict(slots=(0, 1, 2, 0), parent=(0, 1, 2, 3))):
        assert call(**kw) == 1, kw
    assert P(3, 1, 4, 8, ip(sl), 2, ip(sl), 0, 4, kp, None, None) == 1
    S = L.minigpt4_amd_test_beam_select
    s2, step, rt = np.zeros(2, np.float32), np.zeros(44, np.int32), np.zeros(2, np.int32)
    assert S(2, ip(ids[0]), fp(lp[0]), fp(s2), 0, 2, 512, ip(step), ip(rt)) == 1      # no live beam
    assert S(9, ip(ids[0]), fp(lp[0]), fp(s2), 1, 2, 512, ip(step), ip(rt)) == 1
    assert S(2, None, fp(lp[0]), fp(s2), 1, 2, 512, ip(step), ip(rt)) == 1


def test_python_layer_exposes_beam_search():
    from minigpt4_cpp_amd import minigpt4_library as ML
    from minigpt4_cpp_amd import serve as S
    C = ML.MiniGPT4SharedLibrary
    for name in ("amd_beam_search", "amd_test_beam_select_host", "amd_test_beam_select", "amd_test_kv_permute"):
        assert callable(getattr(C, name)), name
    assert inspect.signature(C.amd_beam_search).parameters["length_penalty"].default == 1.0
    assert inspect.signature(S.ReplicaServer.run).parameters["num_beams"].default == 1
