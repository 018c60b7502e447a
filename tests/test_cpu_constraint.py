"""Constrained decoding on the CPU: the pattern compiler (csrc/constraint.cpp, through the test library's hook; no GPU) against tests/constraint_ref.py, an independent
construction.  The minimal trimmed DFA numbered "0 = dead, 1 = start, breadth-first by ascending byte" is unique for a language, so the tables are compared bit for bit.

  1. trans / accepting / S equal the reference's on a set that covers every syntax element; the reference itself equals Python's re.fullmatch on ALL strings up to
     length 6 over 4-letter alphabets, and its dead state is "no enumerated extension matches" where the shortest completions fit that bound;
  2. every refusal, with its byte offset;
  3. regex_escape / choice_pattern round-trip through re and through the compiler."""
import itertools
import re

import numpy as np
import pytest

import constraint_ref as R

E = "é".encode()                                                             # C3 A9


class Pat:
    def __init__(self, name, pattern, alphabets, re_pattern=None, slack=None, longest=None):
        """alphabets: 4-byte strings the enumeration draws from; re_pattern: what Python's re is given where it reads the pattern differently (bytes patterns quantify
        the last BYTE of a multi-byte character; re refuses stacked quantifiers); slack: every live prefix is at most this many alphabet bytes from a match (None: the
        liveness check does not fit the bound); longest: the longest match in bytes (None: unbounded) -- tests/test_gpu_constraint.py decodes the bounded ones."""
        self.name, self.pattern, self.alphabets, self.re_pattern, self.slack, self.longest = name, pattern, alphabets, pattern if re_pattern is None else re_pattern, slack, longest


PATTERNS = [
    Pat("yes_no", b"(yes|no)", [b"yesn", b"noye"], longest=3),
    Pat("digits_1_3", b"[0-9]{1,3}", [b"09a5"], slack=0, longest=3),
    Pat("number", rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?", [b"-0.9", b"01.-"], slack=1),
    Pat("json", rb'\{"n": [0-9]{1,2}, "ok": (true|false)\}', [b'{"n:', b"1, e"], longest=22),
    Pat("no_quote", rb'[^"\n]*', [b'"\na\xff'], slack=0),
    Pat("hex_bytes", rb"\xC3\xA9+", [b"\xc3\xa9a\n"], slack=1),
    Pat("e_acute", E, [b"\xc3\xa9a\n"], slack=1, longest=2),
    Pat("e_acute_plus", E + b"+", [b"\xc3\xa9a\n"], re_pattern=b"(?:" + E + b")+", slack=1),
    Pat("a_0_255", b"a{0,255}", [b"abcd"], slack=0, longest=255),
    Pat("empty_arm", b"(a|)b", [b"ab|c"], slack=1, longest=2),
    Pat("empty", b"", [b"ab\x00\n"], slack=0, longest=0),
    Pat("dot", b"a.c", [b"a\nc."], slack=2, longest=3),
    Pat("bracket_first", b"[]a]+x", [b"]ax["], slack=1),
    Pat("neg_bracket_first", b"[^]a]b", [b"]ab^"], slack=2, longest=2),
    Pat("class_escapes", rb"[\d_\-]+[a\]]", [b"0_-]", b"9a-\\"], slack=2),
    Pat("range_dash_last", b"[a-c-]*d", [b"a-cd", b"bd-e"], slack=1),
    Pat("class_hex", rb"[\x00-\x02\xfe-\xff]{2}", [b"\x00\x02\xfe\xff", b"\x01\x03\xfd\xff"], slack=2, longest=2),
    Pat("word_space", rb"\w+\s\D\W\S", [b"a 1_", b"_\t- "], slack=4),
    Pat("neg_escapes_in_class", rb"[\D][\W\d][^\S]", [b"a1 -"], slack=3, longest=3),
    Pat("non_capture", b"(?:ab)*c", [b"abc("], slack=2),
    Pat("three_arms", b"a|b|", [b"ab|c"], slack=0, longest=1),
    Pat("exact", b"x{2}y{0}z{2,}", [b"xyz{"], slack=4),
    Pat("control_escapes", rb"\n\t|\r\f|\v\0", [b"\n\t\v\x00", b"\r\f\n\t"], slack=2, longest=2),
    Pat("punct_escapes", rb"\.\*\+\?\|\(\)\[\]\{\}\\\^\$\-\"", [b".*+?", b'\\^$"'], longest=16),
    Pat("stacked", b"a**b+*", [b"ab*+"], re_pattern=b"(?:a*)*(?:b+)*", slack=0),
    Pat("nested_counts", b"(ab{1,2}){2,3}", [b"ab{1"], longest=9),
    Pat("alt_in_star", b"(a|bc)*d?", [b"abcd"], slack=1),
    Pat("date", rb"(19|20)\d\d-(0[1-9]|1[0-2])", [b"1920", b"0-12"], longest=7),
    Pat("letters", b"[A-D]", [b"ABDE"], slack=0, longest=1),
    Pat("lone_brackets", b"a]b}", [b"a]b}"], slack=4, longest=4),
]
BY_NAME = {p.name: p for p in PATTERNS}
_REF = {}


def ref_of(p):
    if p.name not in _REF:
        _REF[p.name] = R.compile_ref(p.pattern)
    return _REF[p.name]


def strings(alphabet, max_len=6):
    for n in range(max_len + 1):
        for t in itertools.product(alphabet, repeat=n):
            yield bytes(t)


# ---------------------------------------------------------------------------------------------------------------- 1. the tables
@pytest.mark.parametrize("p", PATTERNS, ids=lambda p: p.name)
def test_compiler_equals_the_reference_bit_for_bit(lib, p):
    trans, acc, S = lib.amd_test_constraint_compile(p.pattern)
    want_t, want_a = ref_of(p)
    assert S == len(want_t), (S, len(want_t))
    assert 2 <= S <= 1024
    assert np.array_equal(trans, want_t)
    assert np.array_equal(acc, R.accept_words(want_a))
    assert not trans[0].any() and not want_a[0]                              # the dead state absorbs and never accepts


def test_the_set_covers_the_issue_patterns_and_state_counts():
    sizes = {p.name: len(ref_of(p)[0]) for p in PATTERNS}
    assert sizes["empty"] == 2 and sizes["a_0_255"] == 257 and sizes["yes_no"] == 6
    assert max(sizes.values()) == 257


@pytest.mark.parametrize("p", PATTERNS, ids=lambda p: p.name)
def test_reference_equals_re_fullmatch_on_all_short_strings(p):
    trans, acc = ref_of(p)
    rx = re.compile(p.re_pattern)
    for alphabet in p.alphabets:
        assert len(alphabet) == 4
        matched = set()
        all_s = list(strings(alphabet))
        for s in all_s:
            got = R.accepts(trans, acc, s)
            assert got == (rx.fullmatch(s) is not None), (p.name, s)
            if got:
                matched.add(s)
        if p.slack is None:
            continue
        has_extension = set()                                                # every prefix of a matching string
        for s in matched:
            for k in range(len(s) + 1):
                has_extension.add(s[:k])
        for s in all_s:
            if len(s) + p.slack <= 6:
                assert (R.walk(trans, R.START, s) != R.DEAD) == (s in has_extension), (p.name, s)
    if p.longest is not None:                                                # the bound the GPU test decodes under
        assert _longest_match(trans, acc) == p.longest


def _longest_match(trans, acc):
    """the longest accepted string of an acyclic automaton (a cycle through a live state: None)"""
    import functools
    import sys
    sys.setrecursionlimit(10000)
    on_path = set()

    @functools.lru_cache(maxsize=None)
    def depth(s):
        if s in on_path:
            raise OverflowError
        on_path.add(s)
        best = 0 if acc[s] else -1
        for t in set(int(x) for x in trans[s]) - {R.DEAD}:
            d = depth(t)
            if d >= 0:
                best = max(best, d + 1)
        on_path.discard(s)
        return best
    try:
        return depth(R.START)
    except OverflowError:
        return None


def test_unbounded_patterns_are_marked_unbounded():
    for p in PATTERNS:
        if p.longest is None:
            assert _longest_match(*ref_of(p)) is None, p.name


# ---------------------------------------------------------------------------------------------------------------- 2. refusals
REFUSALS = [
    (b"(ab", "unbalanced (", 0), (b"a(b", "unbalanced (", 1), (b"ab)", "unbalanced )", 2), (b"a(b|(c)", "unbalanced (", 1),
    (b"a+?", "lazy", 2), (b"a*?", "lazy", 2), (b"a??", "lazy", 2), (b"a*+", "possessive", 2), (b"a{2}?", "lazy", 4), (b"a{2,3}+", "possessive", 6),
    (b"^a", "anchor", 0), (b"a$", "anchor", 1), (b"(a|^b)", "anchor", 3),
    (rb"\q", "escape", 0), (rb"a\1", "escape", 1), (rb"\b", "escape", 0), (rb"ab\A", "escape", 2), (rb"\ ", "escape", 0), (rb"[\q]", "escape", 1),
    (b"a{3,2}", "reversed repeat", 1), (b"a{256}", "above 255", 1), (b"a{1,256}", "above 255", 1), (b"a{,3}", "malformed repeat", 1), (b"a{", "malformed repeat", 1),
    (b"a{2", "malformed repeat", 1), (b"a{x}", "malformed repeat", 1),
    (b"{2}", "nothing to repeat", 0), (b"*a", "nothing to repeat", 0), (b"a|*", "nothing to repeat", 2), (b"(+)", "nothing to repeat", 1),
    (b"[a" + E + b"]", ">= 0x80", 2), (b"[a-" + E + b"]", ">= 0x80", 3), (b"[^" + E + b"]", ">= 0x80", 2),
    (b"(?=a)", "group", 0), (b"(?!a)", "group", 0), (b"x(?<=a)", "group", 1), (b"(?P<n>a)", "group", 0), (b"(?i)a", "group", 0),
    (b"[abc", "unterminated", 0), (b"a[]", "unterminated", 1), (b"[^]", "unterminated", 0), (b"[z-a]", "reversed range", 1), (rb"[a-\d]", "range", 3),
    (rb"\xZ1", "hexadecimal", 0), (rb"a\x4", "hexadecimal", 1), (b"a\\", "trailing backslash", 1),
    (b"\x80", "UTF-8", 0), (b"a\xc3", "UTF-8", 1), (b"\xe2\x82", "UTF-8", 0), (b"\xc3(", "UTF-8", 0), (b"\xff", "UTF-8", 0),
    (b"(" * 251 + b"a" + b")" * 251, "nested", 250),
]


@pytest.mark.parametrize("pattern,word,offset", REFUSALS, ids=lambda v: repr(v)[:24] if isinstance(v, bytes) else None)
def test_refusals_name_the_byte_offset(lib, pattern, word, offset):
    with pytest.raises(ValueError) as e:
        lib.amd_test_constraint_compile(pattern)
    text = str(e.value)
    assert word in text, text
    assert text.endswith(" at byte %d" % offset), text


@pytest.mark.parametrize("pattern,word", [
    (b"(a|b)*a(a|b){12}", "too many states"),                                # 8192 subsets, all distinguishable
    (b"(a|b)*a(a|b){13}", "too many states"),                                # the subset construction's own limit
    (b"(a{255}){255}", "too many states"),                                   # 65 025 positions
    (b"a{255}b{255}c{255}d{255}e{4}", "too many states"),                    # 1026 states: one above the limit
    (rb"[^\x00-\xff]", "matches nothing"), (rb"a[^\x00-\xff]b", "matches nothing"), (rb"(a[^\d\D])+", "matches nothing"),
    (b"a" * 4097, "longer than 4096"),
])
def test_refusals_without_an_offset(lib, pattern, word):
    with pytest.raises(ValueError) as e:
        lib.amd_test_constraint_compile(pattern)
    assert word in str(e.value), str(e.value)


def test_the_limits_themselves_are_accepted(lib):
    assert lib.amd_test_constraint_compile(b"a{255}b{255}c{255}d{255}e{2}")[2] == 1024   # 1022 counted bytes + start + dead... = the largest automaton
    assert lib.amd_test_constraint_compile(b"a**")[2] == 2                   # stacked quantifiers are allowed: a*
    assert lib.amd_test_constraint_compile(b"(" * 250 + b"a" + b")" * 250)[2] == 3
    t, a, S = lib.amd_test_constraint_compile(b"ab\x00c")                     # a NUL byte is a byte (the length is given)
    assert S == 6 and R.accepts(t.astype(np.uint16), np.unpackbits(a.view(np.uint8), bitorder="little")[:S].astype(bool), b"ab\x00c")


# ---------------------------------------------------------------------------------------------------------------- 3. the helpers
TEXTS = ["yes", "a.b", "1+1=2", "(x)", "[y]", "{z}", "a|b", "^$", "back\\slash", "dash-dash", 'say "hi"', "tab\there", "line\nbreak", "caf" + "é", "日本", "a*b?c", " ", "#&~@!%:;,<>/='`_"]


@pytest.mark.parametrize("text", TEXTS, ids=lambda t: repr(t))
def test_regex_escape_round_trips(lib, text):
    from minigpt4_cpp_amd.minigpt4_library import regex_escape
    pat = regex_escape(text)
    data = text.encode()
    assert re.fullmatch(pat.encode(), data) and re.fullmatch(pat, text)
    trans, acc, S = lib.amd_test_constraint_compile(pat)
    assert S == len(data) + 2                                                # a chain: exactly this text
    assert R.walk(trans, R.START, data) == S - 1 and (int(acc[(S - 1) >> 5]) >> ((S - 1) & 31)) & 1
    want_t, want_a = R.compile_ref(pat.encode())
    assert np.array_equal(trans, want_t) and np.array_equal(acc, R.accept_words(want_a))


def test_choice_pattern_matches_exactly_its_options(lib):
    from minigpt4_cpp_amd.minigpt4_library import choice_pattern
    options = ["yes", "no", "n/a", "a.b", "(c)", "1|2", "é"]
    pat = choice_pattern(options)
    trans, acc, S = lib.amd_test_constraint_compile(pat)
    want_t, want_a = R.compile_ref(pat.encode())
    assert np.array_equal(trans, want_t) and np.array_equal(acc, R.accept_words(want_a))
    for o in options:
        assert re.fullmatch(pat, o) and R.accepts(want_t, want_a, o.encode())
    for other in ["", "ye", "yess", "aXb", "c", "1", "12", "\xe9"[:0] + "e"]:
        assert not re.fullmatch(pat, other) and not R.accepts(want_t, want_a, other.encode())
    with pytest.raises(ValueError):
        choice_pattern([])
