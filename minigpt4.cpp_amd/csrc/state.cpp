// Snapshot format version 1 (state.hpp): layout, header, parser.  Host only.
#include "state.hpp"

#include <cstdio>
#include <cstring>

namespace mg4 {

namespace {
constexpr size_t SIZE_LIMIT = (size_t)1 << 46;   // no section comes near: sums of a few terms below it cannot wrap
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
}  // namespace

bool state_layout(const StateHeader &h, StateLayout &l, std::string &why) {
    if (h.n_layer < 1 || h.n_layer > 65536 || h.n_embd < 8 || h.n_embd % 8 || h.n_embd > (1u << 20) || h.n_head < 1 || h.n_vocab < 1 || h.n_vocab > 0x7FFFFFFFu) { why = "bad model shape in the header"; return false; }
    if (h.block_rows < 1) { why = "block_rows is 0"; return false; }
    if (h.n_bias > STATE_BIAS_MAX) { why = "more than 256 logit bias pairs"; return false; }
    if (h.flags & ~(STATE_HAS_LOGITS | STATE_PARITY)) { why = "unknown flag bits"; return false; }
    StateLayout o;
    o.row_bytes = state_row_bytes(h.n_layer, h.n_embd);
    if (o.row_bytes >= SIZE_LIMIT / ((size_t)h.n_rows + 1)) { why = "sizes overflow"; return false; }
    o.n_blocks = (uint32_t)(((uint64_t)h.n_rows + h.block_rows - 1) / h.block_rows);
    o.hist = STATE_HEADER_BYTES;
    o.logits = o.hist + (size_t)4 * h.n_rows;
    o.pen = o.logits + ((h.flags & STATE_HAS_LOGITS) ? (size_t)4 * h.n_vocab : 0);
    o.bias = o.pen + STATE_PEN_BYTES;
    o.table = align_up(o.bias + (size_t)8 * h.n_bias, 8);
    o.kv = align_up(o.table + (size_t)8 * o.n_blocks, 16);
    o.total = o.kv + (size_t)h.n_rows * o.row_bytes;
    l = o;
    return true;
}

void state_write_header(uint8_t *d, const StateHeader &h) {
    memcpy(d, "MG4S", 4);
    state_put32(d + 4, h.version); state_put64(d + 8, h.total_bytes);
    state_put32(d + 16, h.n_layer); state_put32(d + 20, h.n_embd); state_put32(d + 24, h.n_head); state_put32(d + 28, h.n_vocab);
    state_put64(d + 32, h.arena_hash);
    state_put32(d + 40, h.n_rows); state_put32(d + 44, h.block_rows); state_put32(d + 48, h.flags);
    state_put32(d + 52, (uint32_t)h.greedy); state_put32(d + 56, (uint32_t)h.feed); state_put32(d + 60, h.n_bias);
}

bool state_parse(const void *buf, size_t n, StateHeader &out_h, StateLayout &out_l, std::string &why) {
    const uint8_t *p = static_cast<const uint8_t *>(buf);
    if (n == 0 || !p) { why = "empty buffer"; return false; }
    if (n < STATE_HEADER_BYTES) { why = "shorter than the header"; return false; }
    if (memcmp(p, "MG4S", 4) != 0) { why = "wrong magic (not a snapshot)"; return false; }
    StateHeader h;
    h.version = state_get32(p + 4);
    if (h.version != STATE_VERSION) { why = "unsupported version " + std::to_string(h.version); return false; }
    h.total_bytes = state_get64(p + 8);
    if (h.total_bytes != (uint64_t)n) { why = "total size " + std::to_string(h.total_bytes) + " does not match the length " + std::to_string(n); return false; }
    h.n_layer = state_get32(p + 16); h.n_embd = state_get32(p + 20); h.n_head = state_get32(p + 24); h.n_vocab = state_get32(p + 28);
    h.arena_hash = state_get64(p + 32);
    h.n_rows = state_get32(p + 40); h.block_rows = state_get32(p + 44); h.flags = state_get32(p + 48);
    h.greedy = (int32_t)state_get32(p + 52); h.feed = (int32_t)state_get32(p + 56); h.n_bias = state_get32(p + 60);
    StateLayout l;
    if (!state_layout(h, l, why)) return false;
    // section by section against the length, so that the reason names the first one that does not fit
    if (l.logits > n) { why = "token history truncated: " + std::to_string(h.n_rows) + " rows do not fit"; return false; }
    if (l.pen > n) { why = "logits row truncated"; return false; }
    if (l.bias > n || l.bias + (size_t)8 * h.n_bias > n) { why = "penalty parameters or logit bias truncated"; return false; }
    if (l.table > n || l.table + (size_t)8 * l.n_blocks > n) { why = "block table truncated: " + std::to_string(l.n_blocks) + " checksums do not fit"; return false; }
    if (l.total != n) { why = "KV blocks take " + std::to_string(l.total - l.kv) + " bytes from offset " + std::to_string(l.kv) + ", the length is " + std::to_string(n); return false; }
    for (uint32_t r = 0; r < h.n_rows; r++) {
        const int32_t id = (int32_t)state_get32(p + l.hist + (size_t)4 * r);
        if (id < -1 || (int64_t)id >= (int64_t)h.n_vocab) { why = "token history id out of range at row " + std::to_string(r); return false; }
    }
    // what minigpt4_amd_conversation_penalties and minigpt4_amd_set_logit_bias would refuse (bit tests: no float is computed with here)
    auto finite = [](uint32_t bits) { return (bits & 0x7F800000u) != 0x7F800000u; };
    const uint32_t rp = state_get32(p + l.pen + 4);
    if (!finite(rp) || (rp >> 31) || (rp & 0x7FFFFFFFu) == 0) { why = "repeat_penalty must be finite and > 0"; return false; }
    if (!finite(state_get32(p + l.pen + 8)) || !finite(state_get32(p + l.pen + 12))) { why = "alpha_presence and alpha_frequency must be finite"; return false; }
    for (uint32_t b = 0; b < h.n_bias; b++) {
        const int32_t id = (int32_t)state_get32(p + l.bias + (size_t)8 * b);
        if (id < 0 || (int64_t)id >= (int64_t)h.n_vocab) { why = "logit bias id out of range"; return false; }
        const uint32_t v = state_get32(p + l.bias + (size_t)8 * b + 4);
        if (!finite(v) && v != 0xFF800000u) { why = "a logit bias must not be NaN or +infinity"; return false; }
        for (uint32_t a = 0; a < b; a++) if ((int32_t)state_get32(p + l.bias + (size_t)8 * a) == id) { why = "duplicate logit bias id"; return false; }
    }
    if (h.n_rows > 0 || (h.flags & STATE_HAS_LOGITS)) {
        if ((int64_t)h.greedy < 0 || (int64_t)h.greedy >= (int64_t)h.n_vocab || (int64_t)h.feed < 0 || (int64_t)h.feed >= (int64_t)h.n_vocab) { why = "greedy or feed token out of range"; return false; }
    }
    out_h = h; out_l = l;
    return true;
}

}  // namespace mg4

extern "C" int mg4_state_parse(const void *buf, size_t n, int64_t out[12], char *why, size_t why_cap) {
    mg4::StateHeader h; mg4::StateLayout l; std::string w;
    try {
        if (mg4::state_parse(buf, n, h, l, w)) {
            if (out) {
                const int64_t v[12] = {(int64_t)h.version, (int64_t)h.total_bytes, (int64_t)h.n_layer, (int64_t)h.n_embd, (int64_t)h.n_head, (int64_t)h.n_vocab, (int64_t)h.arena_hash,
                                       (int64_t)h.n_rows, (int64_t)h.block_rows, (int64_t)h.flags, (int64_t)h.greedy, (int64_t)h.feed};
                memcpy(out, v, sizeof(v));
            }
            if (why && why_cap) why[0] = 0;
            return 0;
        }
    } catch (...) { w = "out of host memory"; }
    if (why && why_cap) snprintf(why, why_cap, "%s", w.c_str());
    return 1;
}
