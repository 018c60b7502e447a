"""Constrained decoding, restated independently of csrc/constraint.cpp and the kernels: pattern -> syntax tree -> epsilon-NFA -> subset construction -> trim -> minimise ->
canonical numbering (0 = dead, 1 = start, the rest breadth-first from the start by ascending byte), the index bits of every (state, token) and the masked first maximum.
Pure Python / NumPy; byte sets are 256-bit Python integers.  It accepts the syntax include/minigpt4_amd.h states and raises ValueError on anything else (it does not
name offsets: the refusals are the compiler's business)."""
import numpy as np

from test_cpu_penalties import first_max, penalise_ref

ALL = (1 << 256) - 1
DEAD, START, EOS = 0, 1, 2


def _bits(*ranges):
    m = 0
    for lo, hi in ranges:
        for b in range(lo, hi + 1):
            m |= 1 << b
    return m


DIGIT = _bits((0x30, 0x39))
WORD = DIGIT | _bits((0x41, 0x5A), (0x61, 0x7A), (0x5F, 0x5F))
SPACE = sum(1 << b for b in b" \t\n\r\f\v")
CLASS_ESC = {ord("d"): DIGIT, ord("w"): WORD, ord("s"): SPACE, ord("D"): ALL ^ DIGIT, ord("W"): ALL ^ WORD, ord("S"): ALL ^ SPACE}
BYTE_ESC = {ord("n"): 10, ord("t"): 9, ord("r"): 13, ord("f"): 12, ord("v"): 11, ord("0"): 0}
PUNCT = set(range(0x21, 0x30)) | set(range(0x3A, 0x41)) | set(range(0x5B, 0x61)) | set(range(0x7B, 0x7F))


# ------------------------------------------------------------------------------------------------ syntax tree
# ("set", mask) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, lo, hi or None)
class _P:
    def __init__(self, pat):
        self.p, self.i = bytes(pat), 0

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def escape(self):
        """-> (mask, byte or None)"""
        e = self.p[self.i + 1]
        self.i += 2
        if e in CLASS_ESC:
            return CLASS_ESC[e], None
        if e in BYTE_ESC:
            return 1 << BYTE_ESC[e], BYTE_ESC[e]
        if e == ord("x"):
            b = int(self.p[self.i:self.i + 2].decode(), 16)
            self.i += 2
            return 1 << b, b
        if e in PUNCT:
            return 1 << e, e
        raise ValueError("escape")

    def klass(self):
        self.i += 1
        neg = self.peek() == ord("^")
        self.i += neg
        m, first = 0, True
        while True:
            c = self.p[self.i]                                               # IndexError: unterminated
            if c == ord("]") and not first:
                self.i += 1
                break
            first = False
            if c == ord("\\"):
                one, lo = self.escape()
            elif c >= 0x80:
                raise ValueError("class byte")
            else:
                one, lo = 1 << c, c
                self.i += 1
            if lo is not None and self.p[self.i] == ord("-") and self.p[self.i + 1] != ord("]"):
                self.i += 1
                if self.p[self.i] == ord("\\"):
                    _, hi = self.escape()
                else:
                    hi = self.p[self.i]
                    self.i += 1
                if hi is None or hi >= 0x100 or hi < lo:
                    raise ValueError("range")
                one = _bits((lo, hi))
            m |= one
        return ("set", (ALL ^ m) if neg else m)

    def atom(self):
        c = self.peek()
        if c == ord("("):
            self.i += 1
            if self.peek() == ord("?"):
                if self.p[self.i + 1] != ord(":"):
                    raise ValueError("group")
                self.i += 2
            inner = self.alt()
            if self.peek() != ord(")"):
                raise ValueError("unbalanced")
            self.i += 1
            return inner
        if c == ord("["):
            return self.klass()
        if c == ord("."):
            self.i += 1
            return ("set", ALL ^ (1 << 10))
        if c == ord("\\"):
            return ("set", self.escape()[0])
        if c in b"^$*+?{":
            raise ValueError("construct")
        if c < 0x80:
            self.i += 1
            return ("set", 1 << c)
        ch = self.p[self.i:].decode("utf-8", errors="ignore")[:1].encode()   # one UTF-8 character
        if len(ch) < 2 or not self.p.startswith(ch, self.i):
            raise ValueError("utf-8")
        self.i += len(ch)
        return ("cat", [("set", 1 << b) for b in ch])

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in b"|)":
            a = self.atom()
            while self.peek() is not None and self.peek() in b"*+?{":
                q = self.peek()
                if q == ord("{"):
                    end = self.p.index(b"}", self.i)
                    body = self.p[self.i + 1:end].decode()
                    self.i = end + 1
                    lo, sep, hi = body.partition(",")
                    lo = int(lo)
                    hi = lo if not sep else (None if hi == "" else int(hi))
                    if lo > 255 or (hi is not None and not lo <= hi <= 255):
                        raise ValueError("repeat")
                else:
                    self.i += 1
                    lo, hi = {ord("*"): (0, None), ord("+"): (1, None), ord("?"): (0, 1)}[q]
                a = ("rep", a, lo, hi)
                if self.peek() is not None and self.peek() in b"?+":
                    raise ValueError("lazy / possessive")
            items.append(a)
        return items[0] if len(items) == 1 else ("cat", items)

    def alt(self):
        arms = [self.cat()]
        while self.peek() == ord("|"):
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)


def parse(pattern):
    p = _P(pattern)
    try:
        tree = p.alt()
    except (IndexError, KeyError) as e:
        raise ValueError("malformed pattern") from e
    if p.i != len(p.p):
        raise ValueError("unbalanced )")
    return tree


# ------------------------------------------------------------------------------------------------ epsilon-NFA
class _Nfa:
    def __init__(self):
        self.eps, self.edge = [], []                                         # [state] -> [targets]; [state] -> (mask, target) or None

    def new(self):
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def frag(self, node):
        kind = node[0]
        a, z = self.new(), self.new()
        if kind == "set":
            self.edge[a] = (node[1], z)
        elif kind == "cat":
            cur = a
            for k in node[1]:
                s, e = self.frag(k)
                self.eps[cur].append(s)
                cur = e
            self.eps[cur].append(z)
        elif kind == "alt":
            for k in node[1]:
                s, e = self.frag(k)
                self.eps[a].append(s)
                self.eps[e].append(z)
        else:
            _, kid, lo, hi = node
            cur = a
            for _ in range(lo):
                s, e = self.frag(kid)
                self.eps[cur].append(s)
                cur = e
            if hi is None:
                s, e = self.frag(kid)
                self.eps[cur] += [s, z]
                self.eps[e] += [s, z]
            else:
                for _ in range(hi - lo):
                    s, e = self.frag(kid)
                    self.eps[cur] += [s, z]
                    cur = e
                self.eps[cur].append(z)
        return a, z


def _closure(nfa, states):
    seen, todo = set(states), list(states)
    while todo:
        for t in nfa.eps[todo.pop()]:
            if t not in seen:
                seen.add(t)
                todo.append(t)
    return frozenset(seen)


def compile_ref(pattern):
    """-> (trans [S][256] uint16, accepting [S] bool).  ValueError("matches nothing") when the start state is dead."""
    nfa = _Nfa()
    first, last = nfa.frag(parse(pattern))
    # bytes that every edge treats alike share a column
    masks = sorted({e[0] for e in nfa.edge if e is not None})
    column, reps = {}, []
    col_of = []
    for b in range(256):
        key = tuple((m >> b) & 1 for m in masks)
        if key not in column:
            column[key] = len(reps)
            reps.append(b)
        col_of.append(column[key])
    # subset construction
    start = _closure(nfa, [first])
    number, rows, todo = {start: 0}, [], [start]
    while todo:
        cur = todo.pop(0)
        row = []
        for b in reps:
            nxt = _closure(nfa, [nfa.edge[s][1] for s in cur if nfa.edge[s] is not None and (nfa.edge[s][0] >> b) & 1])
            if nxt not in number:
                number[nxt] = len(number)
                todo.append(nxt)
            row.append(number[nxt])
        rows.append(row)                                                     # rows arrive in the order of `number`: a queue
    n = len(rows)
    final = [last in s for s in sorted(number, key=number.get)]
    # trim: the states that reach a final one; every other state is dead
    alive = set(i for i in range(n) if final[i])
    grew = True
    while grew:
        grew = False
        for i in range(n):
            if i not in alive and any(t in alive for t in rows[i]):
                alive.add(i)
                grew = True
    if 0 not in alive:
        raise ValueError("matches nothing")
    dead = n                                                                 # one extra state that absorbs
    step = [[t if t in alive else dead for t in rows[i]] if i in alive else None for i in range(n)] + [[dead] * len(reps)]
    states = sorted(alive) + [dead]
    # minimise: refine {final, not final} by the classes of the successors
    cls = {s: int(s != dead and final[s]) for s in states}
    while True:
        sig = {s: (cls[s],) + tuple(cls[t] for t in step[s]) for s in states}
        names = {}
        for s in states:
            names.setdefault(sig[s], len(names))
        new = {s: names[sig[s]] for s in states}
        if len(names) == len(set(cls.values())):
            break
        cls = new
    # canonical numbering
    one_of = {}
    for s in states:
        one_of.setdefault(cls[s], s)
    num = {cls[dead]: DEAD, cls[0]: START}
    order = [cls[dead], cls[0]]
    q = 1
    while q < len(order):
        s = one_of[order[q]]
        for b in range(256):
            c = cls[step[s][col_of[b]]]
            if c not in num:
                num[c] = len(order)
                order.append(c)
        q += 1
    S = len(order)
    trans, acc = np.zeros((S, 256), np.uint16), np.zeros(S, bool)
    for k in range(1, S):
        s = one_of[order[k]]
        acc[k] = final[s]
        trans[k] = [num[cls[step[s][col_of[b]]]] for b in range(256)]
    return trans, acc


def walk(trans, state, data):
    for b in bytes(data):
        state = int(trans[state, b])
    return state


def accepts(trans, acc, data):
    return bool(acc[walk(trans, START, data)])


def accept_words(acc):
    """the accepting bitmap as the compiler returns it: (S + 31) // 32 little-endian words"""
    pad = np.zeros((len(acc) + 31) // 32 * 32, bool)
    pad[:len(acc)] = acc
    return np.packbits(pad, bitorder="little").view(np.uint32)


# ------------------------------------------------------------------------------------------------ the index and the pick
def index_words(n_vocab):
    return ((n_vocab + 31) // 32 + 3) // 4 * 4


def index_ref(pieces, trans, acc):
    """index[S][W] uint32: bit i of row s.  i >= 3: the piece is not empty and its walk from s does not end in state 0; i == 2: s accepts; ids 0, 1, row 0 and
    the bits at or beyond V: zero."""
    V, S = len(pieces), len(trans)
    lens = np.array([len(p) for p in pieces])
    text = np.zeros((V, max(int(lens.max()), 1)), np.uint8)
    for i, p in enumerate(pieces):
        text[i, :len(p)] = np.frombuffer(bytes(p), np.uint8)
    t32 = trans.astype(np.int32)
    st = np.repeat(np.arange(S, dtype=np.int32)[:, None], V, axis=1)
    for j in range(text.shape[1]):
        on = np.flatnonzero(lens > j)
        st[:, on] = t32[st[:, on], text[on, j][None, :]]
    ok = (st != DEAD) & (lens > 0)[None, :]
    ok[:, :min(3, V)] = False
    if V > EOS:
        ok[:, EOS] = acc
    ok[DEAD, :] = False
    pad = np.zeros((S, index_words(V) * 32), bool)
    pad[:, :V] = ok
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint32).reshape(S, -1)


def allowed_ids(words, n_vocab):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little")[:n_vocab])


def pick_ref(row, words, history=(), n_ctx=4096, bias=(), **pen):
    """(id, stuck): the FIRST maximum of the transformed row (bias, then penalties: penalise_ref) over the allowed ids only; nothing allowed: (EOS, True)."""
    row = np.asarray(row, np.float32)
    ids = allowed_ids(words, len(row))
    if len(ids) == 0:
        return EOS, True
    return int(ids[first_max(penalise_ref(row, list(history), n_ctx, bias=bias, **pen)[ids])]), False
