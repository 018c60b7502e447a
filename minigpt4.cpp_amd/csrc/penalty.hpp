// Repetition / frequency / presence penalties and the logit bias (llama.cpp master-31cfbb1: llama_sample_repetition_penalty,
// llama_sample_frequency_and_presence_penalties, in the order of llama.cpp's main).  ONE definition of the per-entry arithmetic for the host path (sampler.cpp, applied to a
// copy of the row) and for k_pen_pick (llm_kernels.hip): every operation is rounded to fp32 on its own, so the two agree bit for bit.  The host side also builds the table
// the kernel reads: the DISTINCT ids the transformation touches -- the window's ids with their counts, merged with the bias pairs.  Plain host code, no device needed.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MG4_PEN_HD __host__ __device__
#else
#define MG4_PEN_HD
#endif

namespace mg4 {

constexpr int PEN_NL = 13;                       // llama_token_nl() of that llama.cpp
constexpr int PEN_WINDOW_MAX = 1024, PEN_BIAS_MAX = 256;
constexpr int PEN_TABLE_MAX = PEN_WINDOW_MAX + PEN_BIAS_MAX + 1;   // distinct ids one conversation's table can hold
enum : int { PEN_REP = 1, PEN_ALPHA = 2, PEN_KEEP_NL = 4 };       // PenRow::flags: step 3 runs; step 4 runs; the newline id keeps its biased value (step 5)

struct PenParams { int repeat_last_n = 64; float repeat_penalty = 1.0f, alpha_presence = 0.0f, alpha_frequency = 0.0f; int penalize_nl = 1; };   // neutral
struct PenEntry { int id, count; float bias; int has_bias; };      // count: occurrences in the window (0: a bias-only entry)
// what the kernel gets per listed conversation (8 words): logits row, first table entry, entries, flags, the three factors
struct PenRow { int row, off, n, flags; float repeat_penalty, alpha_frequency, alpha_presence; int pad; };

// the window length for a history of `len` rows: the last min(len, W) rows, W = n_ctx when repeat_last_n < 0, clamped to PEN_WINDOW_MAX
inline int pen_window(size_t len, int repeat_last_n, int n_ctx) {
    const int W = std::min(repeat_last_n < 0 ? n_ctx : repeat_last_n, PEN_WINDOW_MAX);
    return (int)std::min(len, (size_t)std::max(W, 0));
}

// The adjusted value of one table entry: bias, then the repetition penalty, then frequency / presence (steps 1, 3, 4; step 5 = the newline id skips 3 and 4).
MG4_PEN_HD inline float pen_value(float l, int id, int count, int has_bias, float bias, int flags, float repeat_penalty, float alpha_frequency, float alpha_presence) {
#if defined(__clang__)
#pragma clang fp contract(off)                   // (the device intrinsics below are plain operators in the default ROCm build: nothing may fuse t = count * f; t + p)
#endif
#if defined(__HIP_DEVICE_COMPILE__)
    if (has_bias) l = __fadd_rn(l, bias);
    if (count <= 0 || ((flags & PEN_KEEP_NL) && id == PEN_NL)) return l;
    if (flags & PEN_REP) l = l <= 0.0f ? __fmul_rn(l, repeat_penalty) : __fdiv_rn(l, repeat_penalty);
    if (flags & PEN_ALPHA) { float t = __fmul_rn((float)count, alpha_frequency); t = __fadd_rn(t, alpha_presence); l = __fsub_rn(l, t); }
    return l;
#else
    if (has_bias) l = l + bias;
    if (count <= 0 || ((flags & PEN_KEEP_NL) && id == PEN_NL)) return l;
    if (flags & PEN_REP) l = l <= 0.0f ? l * repeat_penalty : l / repeat_penalty;
    if (flags & PEN_ALPHA) { float t = (float)count * alpha_frequency; t = t + alpha_presence; l = l - t; }
    return l;
#endif
}

// The table for a history (row-aligned: token id, or -1 for an embedding row -- it takes a place in the window and penalises nothing) and a bias list (distinct ids in
// [0, n_vocab), checked by the caller).  Returns the flags; out = distinct ids, ascending window ids first (counts only while step 3 or 4 runs), then the ids only the
// bias names.  Empty `out` and no flag: the transformation is the identity.
inline int pen_build_table(const int *hist, size_t len, const PenParams &p, int n_ctx, int n_vocab, const int *bias_id, const float *bias_val, int n_bias, std::vector<PenEntry> &out) {
    out.clear();
    const int w = pen_window(len, p.repeat_last_n, n_ctx);
    int flags = 0;
    if (w > 0 && p.repeat_penalty != 1.0f) flags |= PEN_REP;
    if (w > 0 && !(p.alpha_frequency == 0.0f && p.alpha_presence == 0.0f)) flags |= PEN_ALPHA;
    if (flags) {
        std::vector<int> ids;
        ids.reserve((size_t)w);
        for (size_t i = len - (size_t)w; i < len; i++) if (hist[i] >= 0 && hist[i] < n_vocab) ids.push_back(hist[i]);
        std::sort(ids.begin(), ids.end());
        for (size_t i = 0; i < ids.size();) {
            size_t j = i; while (j < ids.size() && ids[j] == ids[i]) j++;
            out.push_back(PenEntry{ids[i], (int)(j - i), 0.0f, 0});
            i = j;
        }
        if (!p.penalize_nl && n_vocab > PEN_NL) flags |= PEN_KEEP_NL;
    }
    const size_t n_win = out.size();
    for (int b = 0; b < n_bias; b++) {
        const auto it = std::lower_bound(out.begin(), out.begin() + (ptrdiff_t)n_win, bias_id[b], [](const PenEntry &e, int id) { return e.id < id; });
        if (it != out.begin() + (ptrdiff_t)n_win && it->id == bias_id[b]) { it->bias = bias_val[b]; it->has_bias = 1; }
        else out.push_back(PenEntry{bias_id[b], 0, bias_val[b], 1});
    }
    return flags;
}

// steps 1-5 on a row of n_vocab logits, in place
inline void pen_apply_row(float *l, int n_vocab, const std::vector<PenEntry> &tab, int flags, const PenParams &p) {
    for (const PenEntry &e : tab)
        if (e.id >= 0 && e.id < n_vocab) l[e.id] = pen_value(l[e.id], e.id, e.count, e.has_bias, e.bias, flags, p.repeat_penalty, p.alpha_frequency, p.alpha_presence);
}

}  // namespace mg4
