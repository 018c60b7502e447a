// Conversation snapshots, format version 1 (include/minigpt4_amd.h documents the layout): the ONE place that reads and writes the header and lays the sections out.
// Host only -- no HIP call, no engine type -- so that the parser is compiled and tested without a GPU (tests/c/state_parse_main.c under AddressSanitizer,
// tests/test_cpu_state.py).  Everything is little-endian and read / written byte by byte: a snapshot may start at any address.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
// The parser behind minigpt4_amd_state_peek, callable from C: the whole buffer is validated (header, section sizes against n, every history and bias id) and out[12] <-
// {version, total bytes, n_layer, n_embd, n_head, n_vocab, arena hash, n_rows, block_rows, flags, greedy token, feed token}.  0, or 1 with the reason (no prefix) in
// why[0 .. why_cap), NUL-terminated; out is then untouched.  buf may be NULL only when n == 0.
int mg4_state_parse(const void *buf, size_t n, int64_t out[12], char *why, size_t why_cap);
#ifdef __cplusplus
}

#include <string>

namespace mg4 {

constexpr uint32_t STATE_VERSION = 1;
constexpr size_t STATE_HEADER_BYTES = 64, STATE_PEN_BYTES = 20, STATE_BLOCK_BYTES_DEFAULT = 32u << 20;
constexpr uint32_t STATE_HAS_LOGITS = 1, STATE_PARITY = 2, STATE_BIAS_MAX = 256;   // flags; the most bias pairs a conversation holds (PEN_BIAS_MAX)

struct StateHeader {                       // byte offset in the file
    uint32_t version = STATE_VERSION;      //  4 (magic "MG4S" at 0)
    uint64_t total_bytes = 0;              //  8
    uint32_t n_layer = 0, n_embd = 0, n_head = 0, n_vocab = 0;   // 16, 20, 24, 28
    uint64_t arena_hash = 0;               // 32
    uint32_t n_rows = 0, block_rows = 1;   // 40, 44
    uint32_t flags = 0;                    // 48
    int32_t greedy = 0, feed = 0;          // 52, 56
    uint32_t n_bias = 0;                   // 60
};
// where the sections lie: history n_rows x i32 | logits n_vocab x f32 (has_logits) | penalties 20 bytes | bias n_bias x (i32, f32) | pad to 8 | block table n_blocks x u64 |
// pad to 16 | KV blocks
struct StateLayout { size_t hist = 0, logits = 0, pen = 0, bias = 0, table = 0, kv = 0, total = 0, row_bytes = 0; uint32_t n_blocks = 0; };

inline size_t state_row_bytes(uint32_t n_layer, uint32_t n_embd) { return (size_t)4 * n_layer * n_embd; }   // K and V, every layer, fp16
inline uint32_t state_block_rows(size_t block_bytes, size_t row_bytes) { const size_t r = row_bytes ? block_bytes / row_bytes : 0; return r < 1 ? 1u : r > 0x7FFFFFFFu ? 0x7FFFFFFFu : (uint32_t)r; }
// rows of block c (the last one may be short)
inline uint32_t state_rows_of_block(const StateHeader &h, uint32_t c) { const uint64_t r0 = (uint64_t)c * h.block_rows; return (uint32_t)(h.n_rows - r0 < h.block_rows ? h.n_rows - r0 : h.block_rows); }
// false + why: a shape no snapshot can have (n_embd % 8, no layer, block_rows 0, too many bias pairs, sizes that overflow)
bool state_layout(const StateHeader &h, StateLayout &l, std::string &why);
void state_write_header(uint8_t *dst, const StateHeader &h);               // STATE_HEADER_BYTES bytes
// header + every host section of buf[0, n) checked; false + why and nothing else written
bool state_parse(const void *buf, size_t n, StateHeader &h, StateLayout &l, std::string &why);

// little-endian scalars at any alignment
inline uint32_t state_get32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t state_get64(const uint8_t *p) { return (uint64_t)state_get32(p) | (uint64_t)state_get32(p + 4) << 32; }
inline void state_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
inline void state_put64(uint8_t *p, uint64_t v) { state_put32(p, (uint32_t)v); state_put32(p + 4, (uint32_t)(v >> 32)); }

}  // namespace mg4
#endif
