#pragma once
// Host-only n-gram drafter of lookup decoding (llama.cpp's lookup example): guesses the next tokens of a sequence from an earlier occurrence of its own suffix.
#include <vector>

namespace mg4 {

class NgramDrafter {
public:
    // suffix lengths tried, longest first: ngram_max ... ngram_min (1 <= ngram_min <= ngram_max)
    NgramDrafter(int ngram_max, int ngram_min) : nmax_(ngram_max), nmin_(ngram_min) {}
    void reset(const int *tokens, int n) { h_.assign(tokens, tokens + (n > 0 ? n : 0)); }
    void push(int id) { h_.push_back(id); }
    int size() const { return (int)h_.size(); }
    // The longest suffix of the history (L tokens, ending in its last token) that also starts at an earlier index s < size - L; among occurrences of that length the
    // most recent (largest s; it may overlap the suffix).  out = the tokens that followed it, h[s + L ...], cut at n_draft tokens, before the first id 2 (</s>) and at
    // the end of the history.  Returns the draft length; 0 = no match (or n_draft < 1).
    int draft(int n_draft, int *out) const;
private:
    int nmax_, nmin_;
    std::vector<int> h_;
};

}  // namespace mg4
