// The row a device pick decides on -- bias and penalties, then the constraint -- as k_pen_pick, k_constrain_pick and k_sample_rows walk it.  Included by llm_kernels.hip
// only, behind RowSpan / row_sweep / argmax_combine / argmax_wave, so the three kernels build with that file's flags.  The transformed row is never materialised: the ids
// of the conversation's table (penalty.hpp: distinct, the ones bias and penalties touch) are MARKED in an LDS bitmap, the row sweep carries the unmarked ids with their
// raw logits, a loop over the table carries the marked ones through pen_value -- the function the host path applies, so both give the same bits.  HAS_ALLOW: a second LDS
// bitmap holds the ids the constraint state allows (a null pointer: every id), and an id whose bit is clear takes part nowhere.  A table id outside [0, n_vocab) is
// ignored everywhere (the host never builds one).  The logits are read in place and never written.
// LDS: words(n_vocab) bitmap words per bitmap, [allow |] marked, at the front of the kernel's dynamic block.  256 threads.
#pragma once

template <bool HAS_ALLOW> struct PickRow {
    const float *x; RowSpan sp; PenRow pr; const PenEntry *tab; int n_vocab; const unsigned *allow; unsigned *marked;
    static __device__ __host__ __forceinline__ int words(int n_vocab) { return constraint_words(n_vocab); }                       // per bitmap
    static __device__ __host__ __forceinline__ int lds_words(int n_vocab) { return (HAS_ALLOW ? 2 : 1) * words(n_vocab); }        // what stage() takes of `lds`
    // THE staging: zero `marked`, load `allow`, mark the table ids; ends behind a barrier
    __device__ __forceinline__ void stage(const float *logits, int ld, int n_vocab_, const PenRow &row, const PenEntry *table, const unsigned *allowed, unsigned *lds, int tid) {
        const int W = words(n_vocab_);
        pr = row; tab = table + (size_t)row.off; n_vocab = n_vocab_; x = logits + (size_t)row.row * ld; sp = row_span(x, n_vocab_);
        unsigned *al = lds; marked = HAS_ALLOW ? lds + W : lds; allow = al;
        for (int i = tid; i < W; i += 256) { if constexpr (HAS_ALLOW) al[i] = allowed ? allowed[i] : 0xFFFFFFFFu; marked[i] = 0u; }
        __syncthreads();
        for (int i = tid; i < pr.n; i += 256) { const int id = tab[i].id; if (id >= 0 && id < n_vocab) atomicOr(&marked[id >> 5], 1u << (id & 31)); }
        __syncthreads();
    }
    __device__ __forceinline__ bool is_allowed(int id) const { if constexpr (HAS_ALLOW) return (allow[id >> 5] >> (id & 31)) & 1u; else return true; }
    __device__ __forceinline__ bool is_marked(int id) const { return (marked[id >> 5] >> (id & 31)) & 1u; }
    __device__ __forceinline__ bool from_row(int id) const {                                                                       // allowed and unmarked
        if constexpr (HAS_ALLOW) return ((allow[id >> 5] & ~marked[id >> 5]) >> (id & 31)) & 1u; else return !is_marked(id);
    }
    // THE value rule of a table entry
    __device__ __forceinline__ float entry_value(const PenEntry &e) const {
        return pen_value(x[e.id], e.id, e.count, e.has_bias, e.bias, pr.flags, pr.repeat_penalty, pr.alpha_frequency, pr.alpha_presence);
    }
    // f(value, id, entry index) for every allowed table id
    template <typename F> __device__ __forceinline__ void each_entry(int tid, F f) const {
        for (int i = tid; i < pr.n; i += 256) {
            const PenEntry e = tab[i];
            if (e.id < 0 || e.id >= n_vocab || !is_allowed(e.id)) continue;
            f(entry_value(e), e.id, i);
        }
    }
    // Every participating id of the transformed row: f(value, id) for the unmarked allowed ids from the row, g(value, id, entry index) for the allowed table ids through
    // pen_value; without g, f takes those too
    template <typename F, typename G> __device__ __forceinline__ void each(int tid, F f, G g) const {
        row_sweep(sp, tid, [&](float v, int i) { if (from_row(i)) f(v, i); });
        each_entry(tid, g);
    }
    template <typename F> __device__ __forceinline__ void each(int tid, F f) const { each(tid, f, [&](float v, int id, int) { f(v, id); }); }
    // the transformed row's value of ONE id in [0, n_vocab): a marked id's entry is looked up in the table (the ids of a table are distinct)
    __device__ __forceinline__ float value_of(int id) const {
        if (is_marked(id)) for (int e = 0; e < pr.n; e++) { const PenEntry pe = tab[e]; if (pe.id == id) return entry_value(pe); }
        return x[id];
    }
};
// The greedy tail, 4 waves: every thread's (best, bi) -> thread 0's first maximum (larger value, then lower id; bi stays 0x7FFFFFFF where no thread carried an id).
// sv, si: 4 entries of LDS each.  Ends behind a barrier.
__device__ __forceinline__ void pick_first_max(float &best, int &bi, int tid, float *sv, int *si) {
    argmax_wave(best, bi);
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) for (int w = 1; w < 4; w++) argmax_combine(best, bi, sv[w], si[w]);
}
// The greedy pick over the transformed row, the one body of k_pen_pick (HAS_ALLOW = false: ONE bitmap) and k_constrain_pick: thread 0 returns the FIRST maximum over the
// participating ids (-0 == +0; an id at -infinity can still win among -infinities; NaN never wins), or `none` when no id takes part.  adjusted (may be null): the value of
// every allowed table entry, at the entry's index of the whole table.  lds: lds_words(n_vocab) bitmap words, then 4 floats and 4 ints of reduction scratch.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): k_pen_pick 17 VGPRs, 46 SGPRs; k_constrain_pick 15 VGPRs, 45 SGPRs; both no scratch, no static LDS,
// occupancy 8 waves per SIMD.
template <bool HAS_ALLOW> __device__ __forceinline__ int pick_greedy(const float *logits, int ld, int n_vocab, const PenRow &row, const PenEntry *table, const unsigned *allowed,
                                                                     float *adjusted, int none, unsigned *lds, int tid) {
    PickRow<HAS_ALLOW> p;
    p.stage(logits, ld, n_vocab, row, table, allowed, lds, tid);
    unsigned *red = lds + PickRow<HAS_ALLOW>::lds_words(n_vocab);
    float best = -INFINITY; int bi = 0x7FFFFFFF;
    auto carry = [&](float v, int i) { argmax_combine(best, bi, v, i); };
    p.each(tid, carry, [&](float v, int id, int i) { if (adjusted) adjusted[(size_t)p.pr.off + i] = v; carry(v, id); });
    pick_first_max(best, bi, tid, reinterpret_cast<float *>(red), reinterpret_cast<int *>(red + 4));
    return bi == 0x7FFFFFFF ? none : bi;
}
