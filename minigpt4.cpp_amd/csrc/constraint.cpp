// Pattern -> minimal byte-level DFA (constraint.hpp states the syntax and the construction).  Plain host code.
#include "constraint.hpp"

#include <algorithm>
#include <bitset>
#include <map>
#include <utility>

namespace mg4 {
namespace {

using ByteSet = std::bitset<256>;
struct Refusal { std::string what; };
[[noreturn]] void refuse_at(const char *what, size_t off) { throw Refusal{std::string(what) + " at byte " + std::to_string(off)}; }
[[noreturn]] void refuse_states(const char *why) { throw Refusal{std::string("too many states: ") + why}; }

constexpr int MAX_DEPTH = 250;                       // nested groups: the parser and the NFA builder recurse once per level

// ---- syntax tree: nodes live in one pool, children by index
struct Node { enum Kind { SET, CAT, ALT, REP } kind = CAT; ByteSet set; std::vector<int> kids; int lo = 0, hi = 0; };   // REP: hi < 0 = unbounded; an empty CAT matches ""

ByteSet range_set(int lo, int hi) { ByteSet s; for (int b = lo; b <= hi; b++) s.set((size_t)b); return s; }
ByteSet class_escape(unsigned char e) {
    ByteSet s;
    switch (e | 0x20) {
    case 'd': s = range_set('0', '9'); break;
    case 'w': s = range_set('0', '9') | range_set('A', 'Z') | range_set('a', 'z'); s.set('_'); break;
    default: for (unsigned char c : {' ', '\t', '\n', '\r', '\f', '\v'}) s.set(c); break;   // 's'
    }
    return (e & 0x20) ? s : ~s;
}
bool is_punct(unsigned char c) { return (c >= 0x21 && c <= 0x2F) || (c >= 0x3A && c <= 0x40) || (c >= 0x5B && c <= 0x60) || (c >= 0x7B && c <= 0x7E); }
int hex_digit(unsigned char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

struct Parser {
    const unsigned char *p; size_t n, pos = 0; int depth = 0;
    std::vector<Node> pool;

    int add(Node nd) { pool.push_back(std::move(nd)); return (int)pool.size() - 1; }
    int add_set(const ByteSet &s) { Node nd; nd.kind = Node::SET; nd.set = s; return add(std::move(nd)); }
    int add_rep(int kid, int lo, int hi) { Node nd; nd.kind = Node::REP; nd.kids = {kid}; nd.lo = lo; nd.hi = hi; return add(std::move(nd)); }

    // pos at the backslash; the set, and whether it is one byte (then `byte`)
    ByteSet escape(bool &single, int &byte) {
        const size_t at = pos;
        if (pos + 1 >= n) refuse_at("trailing backslash", at);
        const unsigned char e = p[pos + 1];
        single = true; pos += 2;
        switch (e) {
        case 'd': case 'w': case 's': case 'D': case 'W': case 'S': single = false; byte = -1; return class_escape(e);
        case 'n': byte = '\n'; break;
        case 't': byte = '\t'; break;
        case 'r': byte = '\r'; break;
        case 'f': byte = '\f'; break;
        case 'v': byte = '\v'; break;
        case '0': byte = 0; break;
        case 'x': {
            const int h = pos < n ? hex_digit(p[pos]) : -1, l = pos + 1 < n ? hex_digit(p[pos + 1]) : -1;
            if (h < 0 || l < 0) refuse_at("\\x needs two hexadecimal digits", at);
            byte = h * 16 + l; pos += 2;
            break;
        }
        default:
            if (!is_punct(e)) refuse_at("unsupported escape", at);
            byte = e;
        }
        return range_set(byte, byte);
    }
    int char_class() {
        const size_t open = pos++;
        bool neg = false, first = true;
        if (pos < n && p[pos] == '^') { neg = true; pos++; }
        ByteSet s;
        for (;;) {
            if (pos >= n) refuse_at("unterminated class", open);
            if (p[pos] == ']' && !first) { pos++; break; }
            first = false;
            const size_t item = pos;
            bool single = true; int lo = 0;
            ByteSet one;
            if (p[pos] == '\\') one = escape(single, lo);
            else if (p[pos] >= 0x80) refuse_at("byte >= 0x80 in a class (write \\xHH)", pos);
            else { lo = p[pos++]; one = range_set(lo, lo); }
            if (single && pos + 1 < n && p[pos] == '-' && p[pos + 1] != ']') {
                pos++;
                bool hs = true; int hi = 0;
                if (p[pos] == '\\') { const size_t at = pos; escape(hs, hi); if (!hs) refuse_at("a class escape cannot end a range", at); }
                else if (p[pos] >= 0x80) refuse_at("byte >= 0x80 in a class (write \\xHH)", pos);
                else hi = p[pos++];
                if (hi < lo) refuse_at("reversed range", item);
                one = range_set(lo, hi);
            }
            s |= one;
        }
        return add_set(neg ? ~s : s);
    }
    // pos at '{': {m} {m,} {m,n}
    void braces(int &lo, int &hi) {
        const size_t open = pos++;
        auto number = [&](int &v) { size_t d = 0; v = 0; while (pos < n && p[pos] >= '0' && p[pos] <= '9' && d < 6) { v = v * 10 + (p[pos++] - '0'); d++; } return d > 0 && d < 6; };
        if (!number(lo)) refuse_at("malformed repeat", open);
        hi = lo;
        if (pos < n && p[pos] == ',') { pos++; if (pos < n && p[pos] == '}') hi = -1; else if (!number(hi)) refuse_at("malformed repeat", open); }
        if (pos >= n || p[pos] != '}') refuse_at("malformed repeat", open);
        pos++;
        if (lo > CONSTRAINT_MAX_REPEAT || hi > CONSTRAINT_MAX_REPEAT) refuse_at("repeat count above 255", open);
        if (hi >= 0 && hi < lo) refuse_at("reversed repeat", open);
    }
    int atom() {
        const unsigned char c = p[pos];
        switch (c) {
        case '(': {
            const size_t open = pos++;
            if (pos < n && p[pos] == '?') { if (pos + 1 < n && p[pos + 1] == ':') pos += 2; else refuse_at("unsupported group construct", open); }
            if (++depth > MAX_DEPTH) refuse_at("groups nested too deeply", open);
            const int inner = alt();
            depth--;
            if (pos >= n || p[pos] != ')') refuse_at("unbalanced (", open);
            pos++;
            return inner;
        }
        case '[': return char_class();
        case '.': { ByteSet s; s.set(); s.reset('\n'); pos++; return add_set(s); }
        case '^': case '$': refuse_at("anchors are not supported (the pattern always matches the whole text)", pos);
        case '*': case '+': case '?': case '{': refuse_at("nothing to repeat", pos);
        case '\\': { bool single; int b; const ByteSet s = escape(single, b); return add_set(s); }
        default: break;
        }
        if (c < 0x80) { pos++; return add_set(range_set(c, c)); }
        const int len = c >= 0xC2 && c <= 0xDF ? 2 : c >= 0xE0 && c <= 0xEF ? 3 : c >= 0xF0 && c <= 0xF4 ? 4 : 0;
        if (!len || pos + (size_t)len > n) refuse_at("malformed UTF-8", pos);
        for (int i = 1; i < len; i++) if ((p[pos + (size_t)i] & 0xC0) != 0x80) refuse_at("malformed UTF-8", pos);
        Node nd; nd.kind = Node::CAT;
        for (int i = 0; i < len; i++) { const int b = p[pos + (size_t)i]; nd.kids.push_back(add_set(range_set(b, b))); }
        pos += (size_t)len;
        return add(std::move(nd));
    }
    int cat() {
        Node nd; nd.kind = Node::CAT;
        while (pos < n && p[pos] != '|' && p[pos] != ')') {
            int a = atom();
            while (pos < n) {
                const unsigned char q = p[pos];
                if (q == '*') { pos++; a = add_rep(a, 0, -1); }
                else if (q == '+') { pos++; a = add_rep(a, 1, -1); }
                else if (q == '?') { pos++; a = add_rep(a, 0, 1); }
                else if (q == '{') { int lo, hi; braces(lo, hi); a = add_rep(a, lo, hi); }
                else break;
                if (pos < n && (p[pos] == '?' || p[pos] == '+')) refuse_at("lazy and possessive quantifiers are not supported", pos);
            }
            nd.kids.push_back(a);
        }
        return nd.kids.size() == 1 ? nd.kids[0] : add(std::move(nd));
    }
    int alt() {
        Node nd; nd.kind = Node::ALT;
        nd.kids.push_back(cat());
        while (pos < n && p[pos] == '|') { pos++; nd.kids.push_back(cat()); }
        return nd.kids.size() == 1 ? nd.kids[0] : add(std::move(nd));
    }
    int parse() {
        const int root = alt();
        if (pos < n) refuse_at("unbalanced )", pos);   // alt() stops only at the end or at a ')' nobody opened
        return root;
    }
};

// ---- Thompson NFA: a state has one byte-set edge or none; epsilon edges are collected flat and indexed afterwards
struct Nfa {
    const std::vector<Node> &pool;
    std::vector<int> set_of, to;                     // [state] index into sets (-1: none), target
    std::vector<ByteSet> sets;                       // distinct
    std::map<std::string, int> set_index;
    std::vector<std::pair<int, int>> eps;
    explicit Nfa(const std::vector<Node> &pool_) : pool(pool_) {}

    int state() {
        if ((int)set_of.size() >= CONSTRAINT_MAX_POSITIONS) refuse_states("the pattern expands to more than 16384 positions");
        set_of.push_back(-1); to.push_back(-1);
        return (int)set_of.size() - 1;
    }
    int intern(const ByteSet &s) {
        std::string key(32, '\0');
        for (int b = 0; b < 256; b++) if (s[(size_t)b]) key[(size_t)b >> 3] = (char)(key[(size_t)b >> 3] | (1 << (b & 7)));
        const auto it = set_index.find(key);
        if (it != set_index.end()) return it->second;
        sets.push_back(s);
        return set_index[key] = (int)sets.size() - 1;
    }
    void link(int a, int b) { eps.emplace_back(a, b); }
    // a fragment (entry, exit); the exit has no outgoing edge yet
    std::pair<int, int> build(int ni) {
        const Node &nd = pool[(size_t)ni];
        const int s = state(), e = state();
        switch (nd.kind) {
        case Node::SET: set_of[(size_t)s] = intern(nd.set); to[(size_t)s] = e; break;
        case Node::CAT: {
            int cur = s;
            for (int k : nd.kids) { const auto f = build(k); link(cur, f.first); cur = f.second; }
            link(cur, e);
            break;
        }
        case Node::ALT:
            for (int k : nd.kids) { const auto f = build(k); link(s, f.first); link(f.second, e); }
            break;
        case Node::REP: {
            int cur = s;
            for (int i = 0; i < nd.lo; i++) { const auto f = build(nd.kids[0]); link(cur, f.first); cur = f.second; }
            if (nd.hi < 0) { const auto f = build(nd.kids[0]); const int hub = state(); link(cur, hub); link(hub, f.first); link(f.second, hub); link(hub, e); }
            else {
                for (int i = nd.lo; i < nd.hi; i++) { const auto f = build(nd.kids[0]); link(cur, f.first); link(cur, e); cur = f.second; }
                link(cur, e);
            }
            break;
        }
        }
        return {s, e};
    }
};

}  // namespace

bool constraint_compile(const unsigned char *pattern, size_t n, ConstraintDfa &out, std::string &err) {
    if (n > (size_t)CONSTRAINT_MAX_PATTERN) { err = "pattern longer than 4096 bytes"; return false; }
    if (n > 0 && !pattern) { err = "no pattern"; return false; }
    try {
        Parser ps{pattern, n};
        const int root = ps.parse();
        Nfa nfa(ps.pool);
        const auto frag = nfa.build(root);
        const int N = (int)nfa.set_of.size(), final_state = frag.second;
        // epsilon edges by source
        std::vector<int> eoff((size_t)N + 1, 0), edst(nfa.eps.size());
        for (const auto &e : nfa.eps) eoff[(size_t)e.first + 1]++;
        for (int i = 0; i < N; i++) eoff[(size_t)i + 1] += eoff[(size_t)i];
        { std::vector<int> fill(eoff.begin(), eoff.end() - 1); for (const auto &e : nfa.eps) edst[(size_t)fill[(size_t)e.first]++] = e.second; }
        // bytes that no set tells apart behave alike everywhere: one column per class
        int cls_of[256], n_cls = 0; std::vector<int> rep;
        {
            std::map<std::vector<bool>, int> seen;
            for (int b = 0; b < 256; b++) {
                std::vector<bool> sig(nfa.sets.size());
                for (size_t k = 0; k < nfa.sets.size(); k++) sig[k] = nfa.sets[k][(size_t)b];
                const auto it = seen.find(sig);
                if (it == seen.end()) { seen[sig] = n_cls; cls_of[b] = n_cls++; rep.push_back(b); } else cls_of[b] = it->second;
            }
        }
        // subset construction; a subset is kept as its states that matter: those with a byte edge, and the final one
        std::vector<int> stamp((size_t)N, -1), stack; int tick = 0;
        auto closure = [&](const std::vector<int> &seed) {
            std::vector<int> key;
            tick++;
            for (int s : seed) if (stamp[(size_t)s] != tick) { stamp[(size_t)s] = tick; stack.push_back(s); }
            while (!stack.empty()) {
                const int s = stack.back(); stack.pop_back();
                if (nfa.set_of[(size_t)s] >= 0 || s == final_state) key.push_back(s);
                for (int k = eoff[(size_t)s]; k < eoff[(size_t)s + 1]; k++) { const int t = edst[(size_t)k]; if (stamp[(size_t)t] != tick) { stamp[(size_t)t] = tick; stack.push_back(t); } }
            }
            std::sort(key.begin(), key.end());
            return key;
        };
        std::map<std::vector<int>, int> ids;
        std::vector<std::vector<int>> subsets, dtrans;   // dtrans[state][class]: raw state, -1 = the empty subset
        std::vector<char> dacc;
        auto intern_subset = [&](std::vector<int> key) {
            if (key.empty()) return -1;
            const auto it = ids.find(key);
            if (it != ids.end()) return it->second;
            if ((int)subsets.size() >= CONSTRAINT_MAX_SUBSETS) refuse_states("the subset construction exceeds 8192 states");
            const int id = (int)subsets.size();
            dacc.push_back(std::binary_search(key.begin(), key.end(), final_state));
            ids[key] = id; subsets.push_back(std::move(key)); dtrans.emplace_back((size_t)n_cls, -1);
            return id;
        };
        intern_subset(closure({frag.first}));            // raw state 0 = start (never empty: the start reaches a byte edge or the final state)
        for (size_t d = 0; d < subsets.size(); d++) {
            for (int c = 0; c < n_cls; c++) {
                std::vector<int> seed;
                for (int s : subsets[d]) if (nfa.set_of[(size_t)s] >= 0 && nfa.sets[(size_t)nfa.set_of[(size_t)s]][(size_t)rep[(size_t)c]]) seed.push_back(nfa.to[(size_t)s]);
                const int t = seed.empty() ? -1 : intern_subset(closure(seed));
                dtrans[d][(size_t)c] = t;
            }
        }
        const int R = (int)subsets.size();
        // trim: raw states that reach an accepting one
        std::vector<char> live((size_t)R, 0);
        {
            std::vector<std::vector<int>> back((size_t)R);
            for (int d = 0; d < R; d++) for (int c = 0; c < n_cls; c++) if (dtrans[(size_t)d][(size_t)c] >= 0) back[(size_t)dtrans[(size_t)d][(size_t)c]].push_back(d);
            std::vector<int> todo;
            for (int d = 0; d < R; d++) if (dacc[(size_t)d]) { live[(size_t)d] = 1; todo.push_back(d); }
            while (!todo.empty()) { const int d = todo.back(); todo.pop_back(); for (int b : back[(size_t)d]) if (!live[(size_t)b]) { live[(size_t)b] = 1; todo.push_back(b); } }
        }
        if (!live[0]) throw Refusal{"matches nothing"};
        // the live states 0 .. M - 1 and the dead state M, complete transition table
        std::vector<int> idx((size_t)R, -1); int M = 0;
        for (int d = 0; d < R; d++) if (live[(size_t)d]) idx[(size_t)d] = M++;
        std::vector<int> t((size_t)(M + 1) * (size_t)n_cls, M); std::vector<char> acc((size_t)M + 1, 0);
        for (int d = 0; d < R; d++) {
            if (!live[(size_t)d]) continue;
            acc[(size_t)idx[(size_t)d]] = dacc[(size_t)d];
            for (int c = 0; c < n_cls; c++) { const int r = dtrans[(size_t)d][(size_t)c]; if (r >= 0 && live[(size_t)r]) t[(size_t)idx[(size_t)d] * (size_t)n_cls + (size_t)c] = idx[(size_t)r]; }
        }
        // minimise (Moore): split blocks by (own block, the blocks of the successors) until nothing splits.  The block count only grows, so one above the limit refuses.
        std::vector<int> block((size_t)M + 1); int n_blocks = 0;
        { bool any_acc = false, any_non = false; for (int s = 0; s <= M; s++) { block[(size_t)s] = acc[(size_t)s] ? 1 : 0; (acc[(size_t)s] ? any_acc : any_non) = true; } n_blocks = (int)any_acc + (int)any_non; }
        for (;;) {
            std::map<std::vector<int>, int> sig_id; std::vector<int> next((size_t)M + 1), sig((size_t)n_cls + 1);
            for (int s = 0; s <= M; s++) {
                sig[0] = block[(size_t)s];
                for (int c = 0; c < n_cls; c++) sig[(size_t)c + 1] = block[(size_t)t[(size_t)s * (size_t)n_cls + (size_t)c]];
                const auto it = sig_id.find(sig);
                if (it == sig_id.end()) { const int id = (int)sig_id.size(); sig_id[sig] = id; next[(size_t)s] = id; } else next[(size_t)s] = it->second;
            }
            const int nb = (int)sig_id.size();
            block.swap(next);
            if (nb > CONSTRAINT_MAX_STATES) refuse_states("the minimal automaton has more than 1024 states");
            if (nb == n_blocks) break;
            n_blocks = nb;
        }
        // canonical numbers: 0 = dead, 1 = start, then breadth-first from the start by ascending byte
        std::vector<int> num((size_t)n_blocks, -1), member((size_t)n_blocks, -1), order;
        for (int s = 0; s <= M; s++) if (member[(size_t)block[(size_t)s]] < 0) member[(size_t)block[(size_t)s]] = s;
        num[(size_t)block[(size_t)M]] = CONSTRAINT_DEAD; order.push_back(M);
        num[(size_t)block[0]] = CONSTRAINT_START; order.push_back(0);   // the start is live, so it is not in the dead state's block
        for (size_t q = 1; q < order.size(); q++) {
            for (int b = 0; b < 256; b++) {
                const int bl = block[(size_t)t[(size_t)order[q] * (size_t)n_cls + (size_t)cls_of[b]]];
                if (num[(size_t)bl] < 0) { num[(size_t)bl] = (int)order.size(); order.push_back(member[(size_t)bl]); }
            }
        }
        const int S = (int)order.size();
        ConstraintDfa dfa;
        dfa.n_states = S; dfa.trans.assign((size_t)S * 256, 0); dfa.accept.assign(((size_t)S + 31) / 32, 0u);
        for (int k = 1; k < S; k++) {
            const int s = order[(size_t)k];
            if (acc[(size_t)s]) dfa.accept[(size_t)k >> 5] |= 1u << (k & 31);
            for (int b = 0; b < 256; b++) dfa.trans[(size_t)k * 256 + (size_t)b] = (uint16_t)num[(size_t)block[(size_t)t[(size_t)s * (size_t)n_cls + (size_t)cls_of[b]]]];
        }
        out = std::move(dfa);
        return true;
    } catch (const Refusal &r) { err = r.what; return false; }
}

}  // namespace mg4
