// Draft verification under sampling, the host's half (include/minigpt4_amd.h states the rule): what the R rows of one verify pass need before k_sample_rows can decide
// them.  Row r of the pass evaluates t_r (t_0 = x0, the conversation's own sample; t_{i + 1} = draft[i]) and its decision x_{r + 1} = D(L_r, h_r, q_r, c + 1 + r) sees
//   h_r = the history followed by t_0 .. t_r        -> one penalty table per row, pen_build_table over the extended history (the window slides with the row)
//   q_r = the constraint state walked over t_0 .. t_r (id 2 leaves it, as Engine::con_walk and minigpt4_amd_constraint_advance do)
// and the draft is CUT at the first token its state does not allow -- the bit k_constrain_index would leave clear in index[q_i]: ids 0 and 1 never, id 2 exactly where q_i
// accepts, any other id when its piece is not empty and its bytes do not lead to the dead state.  A token that cannot be sampled cannot be accepted, so the row behind it
// would be evaluated for nothing.  Plain host code, no device needed (penalty.hpp and beam_host.hpp are the same kind of header); the test hook
// minigpt4_amd_test_draft_tables runs it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "constraint.hpp"
#include "penalty.hpp"

namespace mg4 {

struct DraftStage {
    int n_rows = 0;                              // R = 1 + the draft tokens that stay
    int cut = 0;                                 // draft tokens dropped by the constraint (the caller cuts for room before)
    std::vector<PenRow> rows;                    // [R]: row = r, off = first entry of the row's table in `entries`
    std::vector<PenEntry> entries;               // the R tables back to back
    std::vector<int> state;                      // [R]: q_r; 0 without a constraint
};

// may token `id` be sampled in `state`?  piece(id, &bytes, &n): the token's text; false: no such piece
template <class Piece> inline bool draft_token_allowed(const ConstraintDfa &dfa, int state, int id, Piece &&piece) {
    if (id == CONSTRAINT_EOS) return dfa.accepting(state);
    if (id < 3) return false;
    const unsigned char *b = nullptr; int n = 0;
    if (!piece(id, &b, &n) || n < 1) return false;
    return constraint_walk(dfa.trans.data(), state, b, n) != CONSTRAINT_DEAD;
}
// the state after `id` (EOS, an unknown piece: unchanged)
template <class Piece> inline int draft_state_after(const ConstraintDfa &dfa, int state, int id, Piece &&piece) {
    if (id == CONSTRAINT_EOS) return state;
    const unsigned char *b = nullptr; int n = 0;
    if (!piece(id, &b, &n)) return state;
    return constraint_walk(dfa.trans.data(), state, b, n);
}

// hist[n_hist]: the conversation's row-aligned history as the rows see it (after an automatic shift); draft[n_draft]: already cut to the room left; p: the penalty parameters
// that count (neutral while the mode is off); dfa (may be null: no constraint) and q: the conversation's constraint and its state BEFORE x0.
template <class Piece>
inline void draft_stage(const int *hist, size_t n_hist, int x0, const int *draft, int n_draft, const PenParams &p, const int *bias_id, const float *bias_val, int n_bias,
                        int n_ctx, int n_vocab, const ConstraintDfa *dfa, int q, Piece &&piece, DraftStage &out) {
    out = DraftStage{};
    // 1. the states and the cut
    int state = dfa ? draft_state_after(*dfa, q, x0, piece) : 0, kept = 0;
    out.state.push_back(state);
    for (; kept < n_draft; kept++) {
        if (dfa) {
            if (!draft_token_allowed(*dfa, state, draft[kept], piece)) break;
            state = draft_state_after(*dfa, state, draft[kept], piece);
        }
        out.state.push_back(state);
    }
    out.cut = n_draft - kept;
    out.n_rows = 1 + kept;
    // 2. the tables: only the last PEN_WINDOW_MAX rows of the history can lie in a window
    const size_t tail = n_hist < (size_t)PEN_WINDOW_MAX ? n_hist : (size_t)PEN_WINDOW_MAX;
    std::vector<int> h(hist + (n_hist - tail), hist + n_hist);
    std::vector<PenEntry> tab;
    for (int r = 0; r < out.n_rows; r++) {
        h.push_back(r ? draft[r - 1] : x0);
        const int flags = pen_build_table(h.data(), h.size(), p, n_ctx, n_vocab, bias_id, bias_val, n_bias, tab);
        out.rows.push_back(PenRow{r, (int)out.entries.size(), (int)tab.size(), flags, p.repeat_penalty, p.alpha_frequency, p.alpha_presence, 0});
        out.entries.insert(out.entries.end(), tab.begin(), tab.end());
    }
}

}  // namespace mg4
