#include "draft.hpp"

#include <algorithm>

namespace mg4 {

// A plain scan: n * ngram_max comparisons at worst, microseconds for the few thousand tokens a context holds -- next to a weight pass of milliseconds.
int NgramDrafter::draft(int n_draft, int *out) const {
    const int n = (int)h_.size();
    if (n_draft < 1 || !out || nmin_ < 1) return 0;
    for (int L = std::min(nmax_, n - 1); L >= nmin_; L--) {
        const int *suf = h_.data() + (n - L);
        for (int s = n - L - 1; s >= 0; s--) {
            if (!std::equal(suf, suf + L, h_.data() + s)) continue;
            int m = 0;
            for (int j = s + L; j < n && m < n_draft && h_[(size_t)j] != 2; j++) out[m++] = h_[(size_t)j];
            return m;
        }
    }
    return 0;
}

}  // namespace mg4
