// Beam search, the host's book-keeping around the per-step decision of beam.hpp: token ancestry, the finished list, termination, the rows k_kv_permute has to cover and the
// call's statistics.  Host only (Engine::beam_search and the CPU test hook share it); the length normalisation lives here because it needs powf.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "beam.hpp"

namespace mg4 {

struct BeamHyp { std::vector<int> tok; float score; bool finished; int seq; };   // seq: creation order
// result order: final score descending, then finished before unfinished, then earlier creation first
inline bool beam_hyp_before(const BeamHyp &a, const BeamHyp &b) {
    if (a.score != b.score) return a.score > b.score;
    if (a.finished != b.finished) return a.finished;
    return a.seq < b.seq;
}
inline float beam_final_score(float score, int len, float length_penalty) { return score / powf((float)len, length_penalty); }

struct BeamBook {
    int W, p;                                    // beams; the source's position
    float length_penalty;
    std::vector<std::vector<int>> live_tok;      // tokens of every live beam
    float live_score[BEAM_MAX] = {0};
    std::vector<BeamHyp> done;
    int stats[4] = {0, 0, 0, 0};                 // steps, permute launches that were not the identity, cache rows moved, hypotheses finished by EOS
    int seqno = 0, steps = 0;
    int common;                                  // leading rows known to be identical in all W conversations: the permute of the next step starts here
    bool full = false;                           // the finished list reached W: the search is over
    BeamBook(int W_, int p_, float lp_) : W(W_), p(p_), length_penalty(lp_), live_tok((size_t)W_), common(p_) {}
    // the decision of the step taken at position p + steps (steps tokens emitted so far)
    void step(const BeamStep &r) {
        const int pos = p + steps;
        bool identity = true, same = true;
        int moved = 0;
        for (int i = 0; i < W; i++) { identity = identity && r.parent[i] == i; same = same && r.parent[i] == r.parent[0]; moved += r.parent[i] != i ? 1 : 0; }
        if (!identity && pos > common) { stats[1]++; stats[2] += moved * (pos - common); }
        if (same) common = pos;                  // every conversation now holds that one beam's rows below pos
        for (int f = 0; f < r.n_fin; f++) {
            BeamHyp h{live_tok[(size_t)r.fin_beam[f]], beam_final_score(r.fin_score[f], steps + 1, length_penalty), true, seqno++};
            h.tok.push_back(BEAM_EOS);
            done.push_back(std::move(h)); stats[3]++;
        }
        std::vector<std::vector<int>> next((size_t)W);
        for (int i = 0; i < W; i++) { next[(size_t)i] = live_tok[(size_t)r.parent[i]]; next[(size_t)i].push_back(r.tok[i]); live_score[i] = r.score[i]; }
        live_tok.swap(next);
        steps++; stats[0]++;
        if ((int)done.size() >= W) {             // the list keeps the W best and drops the rest
            std::stable_sort(done.begin(), done.end(), beam_hyp_before);
            done.resize((size_t)W);
            full = true;
        }
    }
    // the end: a search that ran out of steps lets its live beams join, unfinished
    void finish() {
        if (!full) for (int i = 0; i < W; i++) done.push_back(BeamHyp{live_tok[(size_t)i], beam_final_score(live_score[i], steps, length_penalty), false, seqno++});
        std::stable_sort(done.begin(), done.end(), beam_hyp_before);
    }
    // the first min(n_best, hypotheses) rows: tokens_out [n_best][stride] (-1 behind a row's length); returns the count
    int write(int n_best, int stride, int *tokens_out, int *lengths_out, float *scores_out) const {
        const int n = std::min(n_best, (int)done.size());
        for (int i = 0; i < n; i++) {
            const BeamHyp &h = done[(size_t)i];
            lengths_out[i] = (int)h.tok.size(); scores_out[i] = h.score;
            for (int j = 0; j < stride; j++) tokens_out[(size_t)i * stride + j] = j < (int)h.tok.size() ? h.tok[(size_t)j] : -1;
        }
        return n;
    }
};

}  // namespace mg4
