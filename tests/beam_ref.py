"""The beam-search rule of include/minigpt4_amd.h restated in NumPy float32, independent of csrc/beam.hpp and csrc/beam_host.hpp: sorting instead of counting, lists
instead of fixed arrays.  The one thing shared with the library is libm's powf (through ctypes), because the rule names that function."""
import ctypes
import ctypes.util

import numpy as np

EOS = 2
F32 = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def final_score(score, length, length_penalty):
    """score / powf((float)length, length_penalty), one fp32 divide"""
    return F32(F32(score) / F32(_libm.powf(float(length), float(length_penalty))))


def select_step(W, scores, live, ids, lp, eos=EOS):
    """One step.  scores [W] f32, live: iterable of live beam indices, ids / lp [W][2 W] in k_topn_rows' order.
    dict(parent, tok, score: the next live beams; fin: [(beam, raw score)]; margin: score of the last kept candidate minus the first one walked past (None: none left))."""
    C = 2 * W
    cand = []
    for i in sorted(live):
        for c in range(C):
            cand.append((F32(F32(scores[i]) + F32(lp[i][c])), i, c))
    cand.sort(key=lambda x: (-float(x[0]), x[1], x[2]))          # -0.0 and +0.0 compare equal as Python floats too
    parent, tok, score, fin = [], [], [], []
    r_stop = len(cand)
    for r, (s, i, c) in enumerate(cand):
        if len(parent) == W:
            r_stop = r
            break
        if int(ids[i][c]) == eos:
            if r < W:
                fin.append((i, s))
            continue
        parent.append(i); tok.append(int(ids[i][c])); score.append(s)
    margin = None
    if len(cand) > W:
        margin = float(cand[W - 1][0]) - float(cand[W][0])        # the W-th against the (W + 1)-th candidate of the ranking
    return dict(parent=parent, tok=tok, score=score, fin=fin, margin=margin, walked=r_stop)


class Search:
    """The book-keeping of a whole search whose steps are fed from outside: `step(ids, lp)` per step, `finish()` at the end."""

    def __init__(self, W, length_penalty, position=0):
        self.W, self.lpen, self.p = W, length_penalty, position
        self.scores = [F32(0)] + [F32(-np.inf)] * (W - 1)
        self.live = [0]
        self.tokens = [[] for _ in range(W)]
        self.done = []                                            # (final score, finished, creation index, tokens)
        self.created = 0
        self.steps = 0
        self.common = position
        self.permutes = self.rows_moved = self.finished = 0
        self.full = False
        self.log = []

    def step(self, ids, lp):
        W, pos = self.W, self.p + self.steps
        d = select_step(W, self.scores, self.live, ids, lp)
        assert len(d["parent"]) == W, "a step must fill every beam"
        self.log.append(d)
        par = d["parent"]
        if par != list(range(W)) and pos > self.common:
            self.permutes += 1
            self.rows_moved += sum(1 for i in range(W) if par[i] != i) * (pos - self.common)
        if all(q == par[0] for q in par):
            self.common = pos
        for beam, s in d["fin"]:
            self.done.append((final_score(s, self.steps + 1, self.lpen), True, self.created, self.tokens[beam] + [EOS]))
            self.created += 1
            self.finished += 1
        self.tokens = [self.tokens[par[i]] + [d["tok"][i]] for i in range(W)]
        self.scores = list(d["score"])
        self.live = list(range(W))
        self.steps += 1
        if len(self.done) >= W:
            self._sort()
            self.done = self.done[:W]
            self.full = True
        return d

    def _sort(self):
        self.done.sort(key=lambda h: (-float(h[0]), 0 if h[1] else 1, h[2]))

    def finish(self, n_best=None):
        if not self.full:
            for i in range(self.W):
                self.done.append((final_score(self.scores[i], self.steps, self.lpen), False, self.created, list(self.tokens[i])))
                self.created += 1
        self._sort()
        n = self.W if n_best is None else n_best
        return [(np.array(h[3], np.int32), F32(h[0])) for h in self.done[:n]]

    @property
    def stats(self):
        return [self.steps, self.permutes, self.rows_moved, self.finished]


def search_given(ids, lp, length_penalty, n_best=None, position=0):
    """A whole search over given candidates ids / lp [n_steps][W][2 W]: (hypotheses, stats, Search)."""
    T, W, _ = ids.shape
    s = Search(W, length_penalty, position)
    for t in range(T):
        if s.full:
            break
        s.step(ids[t], lp[t])
    return s.finish(n_best), s.stats, s


def pack_step(W, d):
    """The 44-word result block of a step as the library lays it out."""
    out = np.zeros(44, np.int32)
    f = out.view(np.float32)
    out[0:8] = np.arange(8)
    out[0:W] = d["parent"]
    out[8:8 + W] = d["tok"]
    f[16:16 + W] = d["score"]
    out[24], out[25] = W, len(d["fin"])
    out[26:34] = -1
    for k, (beam, s) in enumerate(d["fin"]):
        out[26 + k] = beam
        f[34 + k] = s
    return out
