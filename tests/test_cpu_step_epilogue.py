"""CPU tier of the greedy step-epilogue tests (tests/test_gpu_step_epilogue.py): the numpy reference (tests/greedy_ref.py) against a plain Python loop, the row
builders' own promises, and every refusal of the hooks -- each returns 1 before a device is looked for, so they run without one."""
import math

import numpy as np
import pytest

import greedy_ref as G


def _loop_first_max(row) -> int:
    """The rule, one element at a time: the lowest index holding the largest non-NaN value, when that is above -inf; else 0."""
    best, bi = -math.inf, None
    for i, v in enumerate(np.asarray(row, np.float32).tolist()):
        if v != v:
            continue
        if v > best:
            best, bi = v, i
    return 0 if bi is None else bi


@pytest.mark.parametrize("n", [n for n in G.LENGTHS if n <= 4097] + [16385, 32001])
def test_first_max_is_the_plain_loop(n):
    rows = G.all_rows(n)
    assert len(rows) >= 5
    for label, x, want in rows:
        assert x.dtype == np.float32 and x.shape == (n,)
        assert G.first_max(x) == _loop_first_max(x) == want, (n, label)


def test_first_max_small_cases():
    f = np.float32
    assert G.first_max([f(1), f(3), f(3), f(2)]) == 1
    assert G.first_max([f(-0.0), f(0.0)]) == 0 and G.first_max([f(0.0), f(-0.0)]) == 0
    assert G.first_max([f("nan"), f(2), f("nan"), f(2)]) == 1
    assert G.first_max([f("-inf")] * 3) == 0 and G.first_max([f("nan")] * 3) == 0 and G.first_max([f("nan"), f("-inf"), f("-inf")]) == 0
    assert G.first_max([f("-inf"), f("-inf"), f(-3e38)]) == 2
    assert G.first_max([f("nan"), f("inf"), f("inf")]) == 1


@pytest.mark.parametrize("n", G.LENGTHS)
def test_planted_ties_are_there_and_nothing_else_reaches_the_peak(n):
    pairs = G.tie_pairs(n)
    assert len(set(pairs)) == len(pairs)
    rows = G.tie_rows(n)
    assert len(rows) == len(pairs)
    for (lo, hi), (label, x, want) in zip(pairs, rows):
        assert 0 <= lo < hi < n and want == lo, label
        assert x[lo] == G.PEAK and x[hi] == G.PEAK, label
        rest = np.delete(x, [lo, hi])
        assert np.isfinite(rest).all() and (rest <= G.CAP).all() and G.CAP < G.PEAK, label
    for label, x, want in G.special_rows(n):
        if label.startswith("single"):
            assert (x == G.PEAK).sum() == 1 and x[want] == G.PEAK and (np.delete(x, want) <= G.CAP).all(), label
        if label.startswith(("-0+0", "+0-0")):
            z = np.flatnonzero(x == 0)
            assert len(z) == 2 and z[0] == want and (np.delete(x, z) < 0).all(), label
            assert np.signbit(x[z[0]]) != np.signbit(x[z[1]]) and np.signbit(x[z[0]]) == label.startswith("-0"), label
        if label.startswith("nan_") and label not in ("nan_and_-inf",):
            assert np.isnan(x).any() and not np.isnan(x[want]), label
    if n >= 5:
        sp = {label: (x, want) for label, x, want in G.special_rows(n)}
        x, p = sp["nan_round_peak"]
        assert np.isnan(x[0]) and np.isnan(x[p - 1]) and np.isnan(x[p + 1]) and x[p] == G.PEAK


@pytest.mark.parametrize("kernel", ["argmax", "finish"])
@pytest.mark.parametrize("n", G.LENGTHS + [8, 260, 1028, 1030, 4100, 4101])
def test_tie_pairs_cover_every_compare_the_length_allows(n, kernel):
    got = set()
    for lo, hi in G.tie_pairs(n):
        got |= G.pair_classes(lo, hi, n, kernel)
    want = G.classes_possible(n, kernel)
    assert want <= got, (n, kernel, sorted(want - got))
    assert got <= want | {"f4"}, (n, kernel, sorted(got - want))         # classes_possible is not too modest either


def test_places_follow_the_launch_geometry():
    a = G.argmax_place
    assert a(0)["unit"] == a(16384)["unit"] and a(16384)["trip"] == 1 and a(16383)["group"] == 63 and a(256)["group"] == 1 and a(255)["wave"] == 3
    f = G.finish_place
    assert f(4096, 8192) == dict(group=0, wave=0, lane=0, trip=1, unit=0, f4=0) and f(4095, 8192)["wave"] == 15 and f(7, 8192)["f4"] == 3 and f(7, 8192)["unit"] == 1
    assert f(1024, 2049)["trip"] == 1 and f(1024, 2049)["unit"] == 0 and f(1023, 2049)["wave"] == 15
    # the brute-force view of classes_possible on a length with every class, both kernels: no pair has a class the thresholds do not know
    for kernel, n in (("argmax", 16500), ("finish", 4200), ("finish", 1101)):
        seen = set()
        rng = np.random.default_rng(n)
        for lo, hi in rng.integers(0, n, (4000, 2)):
            if lo != hi:
                seen |= G.pair_classes(int(min(lo, hi)), int(max(lo, hi)), n, kernel)
        assert seen - {"f4"} <= G.classes_possible(n, kernel), (kernel, n, seen)


@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_draft_reference_counts_leading_matches_only(R):
    n = 37
    lg = np.stack([G.planted_row(n, 3000 + r, ((5 * r + 3) % n,)) for r in range(R)])
    ids = [G.first_max(x) for x in lg]
    st = G.start_state(3, n, 1)
    seen = set()
    for m in range(R):
        ref = G.draft_finish_ref(lg, G.draft_toks(ids, m), 2, st)
        assert ref["m"] == m and ref["res"][0] == m and list(ref["res"][1:1 + R]) == ids and (ref["res"][1 + R:] == -1).all()
        assert ref["n_past"][2] == st["n_past"][2] + 1 + m and ref["argmax"][2] == ref["feed"][2] == ids[m]
        assert np.array_equal(ref["slot_logits"][2], lg[m]) and np.array_equal(ref["slot_logits"][[0, 1, 3]], st["slot_logits"][[0, 1, 3]])
        seen.add(m)
    assert seen == set(range(R)) and {0, (R - 1) // 2, R - 1} <= seen                      # 0, a middle value and R - 1
    if R >= 3:
        for m in range(R - 2):
            tok = G.draft_toks(ids, m, later_match=True)
            assert tok[m + 1] != ids[m] and all(tok[i + 1] == ids[i] for i in range(m + 1, R - 1))     # a mismatch, then matches
            assert G.draft_finish_ref(lg, tok, 2, st)["m"] == m                             # which do not count
            assert sum(int(tok[i + 1]) == ids[i] for i in range(R - 1)) > m                 # a count of all matches would differ


@pytest.mark.parametrize("form", [0, 1])
def test_finish_reference_and_slot_maps(form):
    for rows in (1, 2, 5, 64):
        n_slot, n = rows + 3, 9
        for name, sl in G.slot_maps(rows, n_slot, 7).items():
            assert len(set(sl.tolist())) == rows and sl.min() >= 0 and sl.max() < n_slot, name
            assert rows == 1 and sl[0] != 0 or rows > 1 and not (sl == np.arange(rows)).all(), name            # not the identity
            st = G.start_state(n_slot, n, rows)
            for k in ("n_past", "argmax", "feed"):
                assert len(set(st[k].tolist())) == n_slot + 1 and st[k].min() > 1
            lg = np.stack([G.planted_row(n, r, (r % n,)) for r in range(rows)])
            d = sl if form == 0 else np.stack([sl, 500 + 3 * np.arange(rows, dtype=np.int32)], 1)
            ref = G.finish_ref(form, lg, d, st)
            untouched = sorted(set(range(n_slot + 1)) - set(sl.tolist()))
            assert n_slot in untouched and len(untouched) == 4
            for k in st:
                assert np.array_equal(ref[k][untouched], st[k][untouched]), (name, k)
            for r, s in enumerate(sl):
                assert ref["argmax"][s] == ref["feed"][s] == r % n and np.array_equal(ref["slot_logits"][s], lg[r])
                assert ref["n_past"][s] == (st["n_past"][s] + 1 if form == 0 else 500 + 3 * r)


# ---- refusals: 1, before a device is looked for -----------------------------------------------------------------------------------------------------------------------
def _st(n_slot=3, n=8):
    s = G.start_state(n_slot, n, 0)
    return s["n_past"], s["argmax"], s["feed"], s["slot_logits"]


def test_hooks_refuse_bad_arguments_before_any_device(lib):
    import ctypes
    L = lib.library
    npast, am, fd, keep = _st()
    row = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError):
        lib.amd_test_argmax(np.zeros(0, np.float32))
    with pytest.raises(ValueError):
        lib.amd_test_argmax(np.zeros(4, np.float32), n=0)
    out = ctypes.c_int32(7)
    assert L.minigpt4_amd_test_argmax(None, 4, ctypes.byref(out), None, None) == 1 and out.value == 7
    assert L.minigpt4_amd_test_argmax(row.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 4, None, None, None) == 1
    assert L.minigpt4_amd_test_argmax(row.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), (1 << 24) + 1, ctypes.byref(out), None, None) == 1
    # step_finish: form, rows, slots outside [0, n_slot), a slot named twice, fewer slots than rows
    for form, lg, d in [(2, row, [0, 1]), (-1, row, [0, 1]), (0, row, [0, 3]), (0, row, [-1, 1]), (0, row, [1, 1]), (1, row, [[0, 5], [3, 6]]), (1, row, [[2, 5], [2, 6]]),
                        (0, np.zeros((65, 8), np.float32), list(range(65))), (0, np.zeros((4, 8), np.float32), [0, 1, 2, 3])]:
        a, b, c, k = (npast, am, fd, keep) if len(lg) < 65 else _st(80, 8)
        with pytest.raises(ValueError):
            lib.amd_test_step_finish(form, lg, d, a, b, c, k)
    I, F = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    sl = np.array([0, 1], np.int32)
    p = lambda a, t: a.ctypes.data_as(t)
    assert L.minigpt4_amd_test_step_finish(0, None, 2, 8, 3, p(sl, I), p(npast, I), p(am, I), p(fd, I), p(keep, F)) == 1
    assert L.minigpt4_amd_test_step_finish(0, p(row, F), 2, 8, 3, p(sl, I), p(npast, I), p(am, I), p(fd, I), None) == 1
    assert L.minigpt4_amd_test_step_finish(0, p(row, F), 0, 8, 3, p(sl, I), p(npast, I), p(am, I), p(fd, I), p(keep, F)) == 1
    assert L.minigpt4_amd_test_step_finish(0, p(row, F), 2, 0, 3, p(sl, I), p(npast, I), p(am, I), p(fd, I), p(keep, F)) == 1
    # draft_finish: R outside 1 .. 8 is refused here -- the launcher's own throw is never reached -- and so is a slot outside the state
    res = np.zeros(10, np.int32)
    tok = np.zeros(9, np.int32)
    big = np.zeros((9, 8), np.float32)
    for R in (0, 9, -1):
        assert L.minigpt4_amd_test_draft_finish(p(big, F), R, 8, p(tok, I), 3, 1, p(npast, I), p(am, I), p(fd, I), p(keep, F), p(res, I)) == 1
        with pytest.raises(ValueError):
            lib.amd_test_draft_finish(big, tok, 1, npast, am, fd, keep, R=R)
    for slot in (-1, 3):
        with pytest.raises(ValueError):
            lib.amd_test_draft_finish(row, [0, 0], slot, npast, am, fd, keep)
    assert L.minigpt4_amd_test_draft_finish(p(row, F), 2, 8, None, 3, 1, p(npast, I), p(am, I), p(fd, I), p(keep, F), p(res, I)) == 1
    assert L.minigpt4_amd_test_draft_finish(p(row, F), 2, 8, p(tok, I), 3, 1, p(npast, I), p(am, I), p(fd, I), p(keep, F), None) == 1
    assert (res == 0).all()
    # step_words: form, slots, B
    for kw in [dict(form=3, row_slot=[0], n=1), dict(form=0, row_slot=[3], n=1), dict(form=0, row_slot=[-1], n=1), dict(form=1, row_slot=[0, 0], row_pos=[1, 2]),
               dict(form=1, row_slot=[0, 4], row_pos=[1, 2]), dict(form=1, row_slot=[0, 1], row_pos=[1, 2], n=0), dict(form=1, row_slot=[0, 1]),
               dict(form=2, row_slot=[1]), dict(form=2, row_slot=[3], row_pos=[5]), dict(form=1, row_slot=[0, 1, 2, 3], row_pos=[1, 2, 3, 4])]:
        with pytest.raises(ValueError):
            lib.amd_test_step_words(n_past=npast, argmax=am, feed=fd, **kw)
    a, b, c, _ = _st(70, 1)
    with pytest.raises(ValueError):
        lib.amd_test_step_words(1, list(range(65)), a, b, c, row_pos=list(range(65)))
    assert L.minigpt4_amd_test_step_words(0, 3, 1, None, None, 1, p(npast, I), p(am, I), p(fd, I)) == 1
    assert L.minigpt4_amd_test_step_words(0, 3, 1, p(sl, I), None, 1, None, p(am, I), p(fd, I)) == 1
    # gather_rows: an index outside [0, n_src)
    src = np.zeros((3, 5), np.float32)
    for idx in ([3], [0, -1], [0, 1, 2, 7], []):
        with pytest.raises(ValueError):
            lib.amd_test_gather_rows(src, idx)
    with pytest.raises(ValueError):
        lib.amd_test_gather_rows(np.zeros((3, 0), np.float32), [0])
    dst = np.zeros((2, 5), np.float32)
    assert L.minigpt4_amd_test_gather_rows(None, 3, p(sl, I), 1, 5, p(dst, F)) == 1 and L.minigpt4_amd_test_gather_rows(p(src, F), 3, p(sl, I), 1, 5, None) == 1
    assert (dst == 0).all()


def test_hooks_are_test_library_only_and_state_the_rule():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "minigpt4.cpp_amd", "csrc", "test_hooks.cpp")).read()
    test = open(os.path.join(root, "include", "minigpt4_amd_test.h")).read()
    pub = open(os.path.join(root, "include", "minigpt4_amd.h")).read()
    for hook in ("minigpt4_amd_test_argmax(", "minigpt4_amd_test_step_finish(", "minigpt4_amd_test_draft_finish(", "minigpt4_amd_test_step_words(", "minigpt4_amd_test_gather_rows("):
        assert "int " + hook in src and hook in test and hook not in pub, hook
    for text in (src, test):
        assert "lowest index i with row[i] equal to the maximum over the row's non-NaN entries" in " ".join(text.replace("\n * ", " ").replace("\n// ", " ").split())
    from minigpt4_cpp_amd import minigpt4_library as ML
    for name in ("amd_test_argmax", "amd_test_step_finish", "amd_test_draft_finish", "amd_test_step_words", "amd_test_gather_rows"):
        assert callable(getattr(ML.MiniGPT4SharedLibrary, name))
