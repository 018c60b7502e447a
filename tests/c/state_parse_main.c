/* The snapshot parser (minigpt4.cpp_amd/csrc/state.cpp, host only) under AddressSanitizer + UBSan, as a stand-alone C program:
 *   cc -std=c99 -g -fsanitize=address,undefined -c tests/c/state_parse_main.c && c++ -std=c++17 -g -fsanitize=address,undefined -c minigpt4.cpp_amd/csrc/state.cpp
 *   c++ -fsanitize=address,undefined state_parse_main.o state.o -o state_parse && ./state_parse
 * It assembles a valid version-1 snapshot from the layout include/minigpt4_amd.h documents, then feeds the parser: the snapshot (accepted, every field back), EVERY
 * truncation of it -- as it is, and with the header's total-bytes field patched to the shorter length, so that the section checks behind the size check run too --
 * and single-byte corruptions of every header and host-section byte.  Every buffer is an exact-size heap block, so a read past its end is an ASan report.
 * Exit status 0 and "state_parse ok" = every check held. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int mg4_state_parse(const void *buf, size_t n, int64_t out[12], char *why, size_t why_cap);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "state_parse: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

enum { N_LAYER = 2, N_EMBD = 8, N_HEAD = 2, N_VOCAB = 16, N_ROWS = 5, BLOCK_ROWS = 2, N_BIAS = 2, N_BLOCKS = 3, ROW_BYTES = 4 * N_LAYER * N_EMBD };

static void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static void put64(uint8_t *p, uint64_t v) { put32(p, (uint32_t)v); put32(p + 4, (uint32_t)(v >> 32)); }
static void putf(uint8_t *p, float f) { uint32_t u; memcpy(&u, &f, 4); put32(p, u); }

/* the parser on an exact-size copy of buf[0, n) */
static int parse_copy(const uint8_t *buf, size_t n, int64_t out[12], char *why, size_t cap) {
    uint8_t *c = (uint8_t *)malloc(n ? n : 1);
    if (!c) { fprintf(stderr, "state_parse: out of memory\n"); exit(2); }
    if (n) memcpy(c, buf, n);
    const int rc = mg4_state_parse(n ? c : NULL, n, out, why, cap);
    free(c);
    return rc;
}

int main(void) {
    const size_t hist = 64, logits = hist + 4 * N_ROWS, pen = logits + 4 * N_VOCAB, bias = pen + 20, table = (bias + 8 * N_BIAS + 7) / 8 * 8,
                 kv = (table + 8 * N_BLOCKS + 15) / 16 * 16, total = kv + (size_t)N_ROWS * ROW_BYTES;
    uint8_t *s = (uint8_t *)calloc(total, 1);
    CHECK(s);
    memcpy(s, "MG4S", 4);
    put32(s + 4, 1); put64(s + 8, total);
    put32(s + 16, N_LAYER); put32(s + 20, N_EMBD); put32(s + 24, N_HEAD); put32(s + 28, N_VOCAB);
    put64(s + 32, 0xFEDCBA9876543210ull);
    put32(s + 40, N_ROWS); put32(s + 44, BLOCK_ROWS); put32(s + 48, 1 | 2);
    put32(s + 52, 7); put32(s + 56, 9); put32(s + 60, N_BIAS);
    const int32_t ids[N_ROWS] = {1, -1, -1, 15, 3};
    for (int r = 0; r < N_ROWS; r++) put32(s + hist + 4 * r, (uint32_t)ids[r]);
    for (int i = 0; i < N_VOCAB; i++) putf(s + logits + 4 * i, 0.25f * (float)i - 1.0f);
    put32(s + pen, 64); putf(s + pen + 4, 1.3f); putf(s + pen + 8, 0.0f); putf(s + pen + 12, 0.5f); put32(s + pen + 16, 1);
    put32(s + bias, 4); putf(s + bias + 4, -2.0f); put32(s + bias + 8, 11); putf(s + bias + 12, 1.5f);
    for (size_t i = kv; i < total; i++) s[i] = (uint8_t)(i * 37u + 11u);
    for (int c = 0; c < N_BLOCKS; c++) {   /* the table: the wrapping 64-bit sum of each block's 32-bit words */
        const size_t b0 = kv + (size_t)c * BLOCK_ROWS * ROW_BYTES, rows = c == N_BLOCKS - 1 ? N_ROWS - c * BLOCK_ROWS : BLOCK_ROWS;
        uint64_t sum = 0;
        for (size_t w = 0; w < rows * ROW_BYTES / 4; w++) { const uint8_t *p = s + b0 + 4 * w; sum += (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
        put64(s + table + 8 * c, sum);
    }

    int64_t out[12]; char why[256];
    /* 1. accepted, every field back */
    CHECK(parse_copy(s, total, out, why, sizeof(why)) == 0 && why[0] == 0);
    const int64_t want[12] = {1, (int64_t)total, N_LAYER, N_EMBD, N_HEAD, N_VOCAB, (int64_t)0xFEDCBA9876543210ull, N_ROWS, BLOCK_ROWS, 3, 7, 9};
    for (int i = 0; i < 12; i++) CHECK(out[i] == want[i]);
    CHECK(mg4_state_parse(s, total, NULL, NULL, 0) == 0);                       /* no output wanted */
    /* 2. every truncation, as it is and with the total field patched: refused with a reason, out untouched */
    int refused = 0;
    for (size_t n = 0; n < total; n++) {
        for (int patched = 0; patched < 2; patched++) {
            uint8_t *t = (uint8_t *)malloc(n ? n : 1);
            CHECK(t);
            if (n) memcpy(t, s, n);
            if (patched && n >= 16) put64(t + 8, n);
            int64_t o2[12]; for (int i = 0; i < 12; i++) o2[i] = -77;
            why[0] = 0;
            CHECK(mg4_state_parse(n ? t : NULL, n, o2, why, sizeof(why)) == 1);
            CHECK(why[0] != 0);
            for (int i = 0; i < 12; i++) CHECK(o2[i] == -77);
            free(t);
            refused++;
        }
    }
    /* the reasons name the first section that does not fit */
    { uint8_t t[64 + 8]; memcpy(t, s, sizeof(t)); put64(t + 8, sizeof(t)); CHECK(parse_copy(t, sizeof(t), out, why, sizeof(why)) == 1 && strstr(why, "history")); }
    { uint8_t *t = (uint8_t *)malloc(table + 8); CHECK(t); memcpy(t, s, table + 8); put64(t + 8, table + 8); CHECK(parse_copy(t, table + 8, out, why, sizeof(why)) == 1 && strstr(why, "block table")); free(t); }
    CHECK(parse_copy(s, 0, out, why, sizeof(why)) == 1 && strstr(why, "empty"));
    /* a reason longer than the caller's buffer is cut, with the NUL inside it */
    { char tiny[4] = {'x', 'x', 'x', 'x'}; CHECK(parse_copy(s, total - 1, out, tiny, sizeof(tiny)) == 1 && tiny[3] == 0); }
    /* 3. single-byte corruptions of the header and the host sections: any verdict, no bad access; an accepted one still describes a buffer of this length */
    int accepted = 0;
    const uint8_t flips[3] = {0xFF, 0x01, 0x80};
    for (size_t i = 0; i < kv; i++) {
        for (int f = 0; f < 3; f++) {
            s[i] ^= flips[f];
            const int rc = parse_copy(s, total, out, why, sizeof(why));
            CHECK(rc == 0 || rc == 1);
            if (rc == 0) { accepted++; CHECK(out[1] == (int64_t)total); } else CHECK(why[0] != 0);
            s[i] ^= flips[f];
        }
    }
    /* a magic, version or total-bytes byte can never be flipped unnoticed */
    for (size_t i = 0; i < 16; i++) { s[i] ^= 0x01; CHECK(parse_copy(s, total, out, why, sizeof(why)) == 1); s[i] ^= 0x01; }
    CHECK(parse_copy(s, total, out, why, sizeof(why)) == 0);                    /* restored */
    free(s);
    printf("state_parse ok: %d truncations refused, %d of %d corruptions still well-formed\n", refused, accepted, (int)(3 * kv));
    return 0;
}
