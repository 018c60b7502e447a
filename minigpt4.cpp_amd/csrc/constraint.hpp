// Constrained decoding: a regular expression per conversation, compiled ONCE to a byte-level DFA (constraint.cpp, plain host code, no device needed).  The generated text --
// the concatenated bytes of the picked tokens -- must match the WHOLE pattern.  One definition of the token walk for the host (Engine::constraint_advance, the walk after
// every constrained pick) and for k_constrain_index (llm_kernels.hip), which builds the bitmap of allowed tokens of every DFA state.
//
// Syntax (bytes; any other construct is refused with its byte offset):
//   literal byte; a multi-byte UTF-8 character outside a class is its byte sequence and a quantifier behind it applies to the whole character
//   .            any byte except 0x0A
//   [...] [^...] ranges; a ']' in first place is a literal; escapes are allowed inside; a byte >= 0x80 inside is refused (write \xHH)
//   ( ) (?: )    groups, no capture;   |   alternation, empty alternatives allowed
//   * + ? {m} {m,} {m,n}   0 <= m <= n <= 255; quantifiers stack (a** is a*), a '?' or '+' behind a quantifier (lazy / possessive) is refused
//   \d \w \s \D \W \S   ASCII classes, the negations range over all 256 bytes;   \n \t \r \f \v \0 \xHH;   \ + ASCII punctuation: that byte
//   refused: anchors, back-references, look-around and every other (? group, \ + any other letter or digit, a bare quantifier, groups nested deeper than 250
// '.' and negated classes match ONE BYTE, not one character: [^"]* admits any byte sequence without a quote, well-formed UTF-8 or not.
//
// Construction: Thompson NFA with counted repeats expanded (at most CONSTRAINT_MAX_POSITIONS states), subset construction (at most CONSTRAINT_MAX_SUBSETS), trim (every state
// that cannot reach an accepting one becomes THE dead state), minimise, renumber: 0 = dead, 1 = start, the rest breadth-first from the start by ascending byte.  The
// minimal trimmed DFA numbered this way is unique for a language.  Result: trans[S][256] and an accepting bitmap, 2 <= S <= CONSTRAINT_MAX_STATES; row 0 is all zero.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MG4_CON_HD __host__ __device__
#else
#define MG4_CON_HD
#endif

namespace mg4 {

constexpr int CONSTRAINT_MAX_PATTERN = 4096, CONSTRAINT_MAX_POSITIONS = 16384, CONSTRAINT_MAX_SUBSETS = 8192, CONSTRAINT_MAX_STATES = 1024, CONSTRAINT_MAX_REPEAT = 255;
constexpr int CONSTRAINT_DEAD = 0, CONSTRAINT_START = 1, CONSTRAINT_EOS = 2;   // token ids 0 and 1 are never allowed, 2 (EOS) exactly in an accepting state

struct ConstraintDfa {
    int n_states = 0;
    std::vector<uint16_t> trans;                     // [n_states][256]
    std::vector<uint32_t> accept;                    // (n_states + 31) / 32 words
    bool accepting(int s) const { return s >= 0 && s < n_states && ((accept[(size_t)s >> 5] >> (s & 31)) & 1u); }
};

// false + err ("... at byte N" for a syntax refusal; "too many states ..."; "matches nothing"; "pattern longer than 4096 bytes"), out untouched
bool constraint_compile(const unsigned char *pattern, size_t n, ConstraintDfa &out, std::string &err);

// words of one index row (k_constrain_index) for a vocabulary: (n_vocab + 31) / 32 rounded up to 4
MG4_CON_HD inline int constraint_words(int n_vocab) { return ((n_vocab + 31) / 32 + 3) & ~3; }
// the token walk: the left fold of trans over a piece's bytes (unsigned; a NUL byte is a byte).  State 0 absorbs.
MG4_CON_HD inline int constraint_walk(const uint16_t *trans, int state, const unsigned char *bytes, int n) {
    for (int i = 0; i < n && state; i++) state = trans[(size_t)state * 256 + bytes[i]];
    return state;
}

}  // namespace mg4
