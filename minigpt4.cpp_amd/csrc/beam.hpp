// Beam search, one step of the rule (include/minigpt4_amd.h states it): ONE definition for k_beam_select (llm_kernels.hip), which decides every step of
// Engine::beam_search in both modes, and for the host (the CPU test hook the kernel is held against), as penalty.hpp is for the penalties.  Plain C++ without a library call, so both compilers see the same operations.
//   candidates  (i, c): beam i < W, c < C -- the c-th best token of beam i in k_topn_rows' order -- of the LIVE beams; flat index j = i * C + c
//   score       s[i] + lp[i][c], one fp32 add (nothing to fuse: both operands come from memory)
//   ranking     score descending; equal scores (float equality: -0 and +0 tie) by ascending j, i.e. ascending beam, then ascending c
//   walk        in ranking order: an EOS candidate at a rank below W finishes a hypothesis (beam, raw score -- the length normalisation is the host's, it needs powf), an
//               EOS candidate at rank >= W is skipped, any other candidate becomes the next live beam until W are filled
// The ranking is done by counting predecessors (beam_rank_of: one thread per candidate on the device, a loop on the host), the walk by one thread.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MG4_BEAM_HD __host__ __device__
#else
#define MG4_BEAM_HD
#endif

namespace mg4 {

constexpr int BEAM_MAX = 8;                      // beams per search
constexpr int BEAM_CAND_MAX = 2 * BEAM_MAX;      // C = min(2 W, n_vocab) candidates per beam
constexpr int BEAM_EOS = 2;                      // llama_token_eos(): the id minigpt4_amd_token_piece prints as "</s>"

// what one step decides (the device result block has exactly this layout: 44 words)
struct BeamStep {
    int parent[BEAM_MAX];                        // next live beam i continues beam parent[i] ...
    int tok[BEAM_MAX];                           // ... with this token ...
    float score[BEAM_MAX];                       // ... at this cumulative score
    int n_live;                                  // live beams filled (W whenever n_vocab > 2 W)
    int n_fin;                                   // hypotheses finished by EOS in this step, in walk order
    int fin_beam[BEAM_MAX];                      // the beam each of them extends
    float fin_score[BEAM_MAX];                   // its raw score (EOS included)
    int pad[2];
};
static_assert(sizeof(BeamStep) == 44 * 4, "the result block is copied as words");

MG4_BEAM_HD inline float beam_score(float s, float lp) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(s, lp);
#else
    return s + lp;
#endif
}
// does candidate (sa, ja) rank before candidate (sb, jb)?
MG4_BEAM_HD inline bool beam_before(float sa, int ja, float sb, int jb) { return sa > sb || (sa == sb && ja < jb); }
// the rank of candidate j among the candidates of the live beams (live: bit i = beam i is live); cand[] holds every flat index's score
MG4_BEAM_HD inline int beam_rank_of(int j, const float *cand, int W, int C, unsigned live) {
    int r = 0;
    const float sj = cand[j];
    for (int i = 0; i < W; i++) {
        if (!((live >> i) & 1u)) continue;
        for (int c = 0; c < C; c++) r += beam_before(cand[i * C + c], i * C + c, sj, j) ? 1 : 0;
    }
    return r;
}
// the walk over order[0 .. n_cand) (flat indices in ranking order)
MG4_BEAM_HD inline void beam_walk(const int *order, int n_cand, const int *ids, const float *cand, int W, int C, int eos, BeamStep &out) {
    int nl = 0, nf = 0;
    for (int i = 0; i < BEAM_MAX; i++) { out.parent[i] = i; out.tok[i] = 0; out.score[i] = 0.0f; out.fin_beam[i] = -1; out.fin_score[i] = 0.0f; }
    out.pad[0] = out.pad[1] = 0;
    for (int r = 0; r < n_cand && nl < W; r++) {
        const int j = order[r], beam = j / C;
        if (j < 0) continue;                     // a rank no candidate took (NaN scores): nothing is indexed with it
        if (ids[j] == eos) {
            if (r < W && nf < BEAM_MAX) { out.fin_beam[nf] = beam; out.fin_score[nf] = cand[j]; nf++; }
            continue;
        }
        out.parent[nl] = beam; out.tok[nl] = ids[j]; out.score[nl] = cand[j]; nl++;
    }
    out.n_live = nl; out.n_fin = nf;
}
// the whole step on one thread (host; the kernel spreads the first two loops over its threads)
inline void beam_select_host(int W, int C, const float *s, unsigned live, const int *ids, const float *lp, int eos, BeamStep &out) {
    float cand[BEAM_MAX * BEAM_CAND_MAX];
    int order[BEAM_MAX * BEAM_CAND_MAX];
    int n_cand = 0;
    for (int j = 0; j < W * C; j++) order[j] = -1;
    for (int j = 0; j < W * C; j++) cand[j] = beam_score(s[j / C], lp[j]);
    for (int j = 0; j < W * C; j++) {
        if (!((live >> (j / C)) & 1u)) continue;
        order[beam_rank_of(j, cand, W, C, live)] = j;
        n_cand++;
    }
    beam_walk(order, n_cand, ids, cand, W, C, eos, out);
}

}  // namespace mg4
