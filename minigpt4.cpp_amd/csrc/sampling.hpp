// Device-side sampling of batched decode steps (include/minigpt4_amd.h states the rule): ONE definition of the generator and of the rule's arithmetic for k_sample_rows
// (llm_kernels.hip), whose thread 0 runs it over the candidates the workgroup selected, and for the host (the CPU test hook the kernel is held against), as penalty.hpp is
// for the penalties and beam.hpp for the beam step.
//   generator   Philox4x32-10 (Random123): key = (seed low word, seed high word), counter = (draw low, draw high, 0, 0); the draw uses output word 0.  Counter-based: draw k
//               of seed s is the same word whichever conversations share the step and wherever the conversation stands in the slot list.
//   candidates  v[0 .. n_c), value descending, equal values by ascending id (k_topn_rows' order), n_c <= SAMPLE_MAX
//   arithmetic  fp32, each operation rounded on its own (nothing fused), sequential in candidate order -- llama.cpp's top-k -> top-p -> temperature -> softmax -> draw:
//     1. top_p < 1: a_j = expf(v_j - v_0), A = sum a_j, q_j = a_j / A, c += q_j; kept = the first j + 1 with c >= top_p (none: n_c).  top_p >= 1: kept = n_c
//     2. w_j = v_j / temp, j < kept
//     3. b_j = expf(w_j - w_0), S_j = the running sum, S = S_{kept - 1}; reported p_j = b_j / S
//     4. u = (float)(word >> 8) * 2^-24, t = u * S, pick = the first j with S_j > t (none -- u * S can round up to S --: kept - 1)
// No local array: b_j is kept in p[] (LDS on the device), the running sums are recomputed in the same order with the same roundings.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MG4_SMP_HD __host__ __device__
#else
#define MG4_SMP_HD
#endif

namespace mg4 {

constexpr int SAMPLE_MAX = 64;                   // candidates per decision: top_k in 1 .. 64 (covers the reference's default of 40)

// what one decision reports (133 words; the device result block is an array of these)
struct SampleOut {
    int pick, stuck;                             // the sampled id; 1: no id took part, pick = CONSTRAINT_EOS
    unsigned word;                               // the Philox output word the draw used
    int n_cand, kept;                            // candidates selected (min(top_k, participating ids)), candidates left by top-p
    int ids[SAMPLE_MAX];                         // the candidates in order, -1 behind n_cand
    float p[SAMPLE_MAX];                         // their probabilities, 0 behind kept
};

MG4_SMP_HD inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// the word of draw `draws` of `seed`
MG4_SMP_HD inline uint32_t sample_word(uint64_t seed, uint64_t draws) {
    const uint32_t ctr[4] = {(uint32_t)draws, (uint32_t)(draws >> 32), 0u, 0u}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t out[4];
    philox4x32_10(ctr, key, out);
    return out[0];
}

namespace smp {   // one rounding per operation on both sides (the device intrinsics are plain operators in the default ROCm build; nothing may fuse)
#if defined(__HIP_DEVICE_COMPILE__)
MG4_SMP_HD inline float add(float a, float b) { return __fadd_rn(a, b); }
MG4_SMP_HD inline float sub(float a, float b) { return __fsub_rn(a, b); }
MG4_SMP_HD inline float mul(float a, float b) { return __fmul_rn(a, b); }
MG4_SMP_HD inline float div(float a, float b) { return __fdiv_rn(a, b); }
#else
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
inline float add(float a, float b) { return a + b; }
inline float sub(float a, float b) { return a - b; }
inline float mul(float a, float b) { return a * b; }
inline float div(float a, float b) { return a / b; }
#endif
}  // namespace smp

// steps 1 to 4 on v[0 .. n_c), 1 <= n_c <= SAMPLE_MAX, temp > 0, 0 < top_p: the index of the picked candidate; p[0 .. n_c) = the probabilities (0 from kept on), *kept_out
MG4_SMP_HD inline int sample_rule(const float *v, int n_c, float temp, float top_p, uint32_t word, float *p, int *kept_out) {
    int kept = n_c;
    if (top_p < 1.0f) {
        float A = 0.0f;
        for (int j = 0; j < n_c; j++) A = smp::add(A, expf(smp::sub(v[j], v[0])));
        float c = 0.0f;
        for (int j = 0; j < n_c; j++) {
            c = smp::add(c, smp::div(expf(smp::sub(v[j], v[0])), A));
            if (c >= top_p) { kept = j + 1; break; }
        }
    }
    const float w0 = smp::div(v[0], temp);
    float S = 0.0f;
    for (int j = 0; j < kept; j++) { p[j] = expf(smp::sub(smp::div(v[j], temp), w0)); S = smp::add(S, p[j]); }
    const float u = smp::mul((float)(word >> 8), 5.9604644775390625e-8f), t = smp::mul(u, S);
    int pick = kept - 1;
    float run = 0.0f;
    for (int j = 0; j < kept; j++) { run = smp::add(run, p[j]); if (run > t) { pick = j; break; } }
    for (int j = 0; j < kept; j++) p[j] = smp::div(p[j], S);
    for (int j = kept; j < n_c; j++) p[j] = 0.0f;
    *kept_out = kept;
    return pick;
}

// ---- the extended rule (include/minigpt4_amd.h: tail-free -> typical -> top-p -> min-p -> temperature -> softmax -> draw over the live list L, or mirostat v2 behind
// top-k).  sample_rule and SampleOut above are the plain rule's and stay as they are; with tfs_z = typical_p = 1, min_p = 0, mirostat = 0 sample_chain performs exactly
// sample_rule's operations in its order, so pick, kept and every bit of p are the same.
struct ChainParams { float tfs_z, typical_p, min_p; int mirostat; float tau, eta, mu; int pad; };   // 8 words; mu NaN: unset (2 * tau at a mirostat decision)
struct ChainRes { int pick, kept; unsigned mask_lo, mask_hi; float mu, observed; };                  // pick: candidate index; kept = |L|; mask bit j: candidate j is in L
// a descriptor / result of the extended device decision: the plain one, then the chain's words (26 / 137 words)
struct SampleOutEx { SampleOut base; unsigned mask_lo, mask_hi; float mu, observed; };

#if defined(__HIP_DEVICE_COMPILE__)
#define MG4_SMP_SYNC() __syncthreads()
#else
#define MG4_SMP_SYNC() ((void)0)
#endif

// a_j = expf(v_j - v_first(L)) into a[0 .. m), j in list order; returns their sequential sum
MG4_SMP_HD inline float chain_softmax(const float *v, const int *L, int m, float *a) {
    const float v0 = v[L[0]];
    float A = 0.0f;
    for (int j = 0; j < m; j++) { a[j] = expf(smp::sub(v[L[j]], v0)); A = smp::add(A, a[j]); }
    return A;
}
// the draw of step 5 over b[0 .. m) with running sum S: the first position whose running sum exceeds u * S, m - 1 if none
MG4_SMP_HD inline int chain_draw(const float *b, int m, float S, uint32_t word) {
    const float u = smp::mul((float)(word >> 8), 5.9604644775390625e-8f), t = smp::mul(u, S);
    float run = 0.0f;
    for (int j = 0; j < m; j++) { run = smp::add(run, b[j]); if (run > t) return j; }
    return m - 1;
}

// The extended rule on v[0 .. n_c), 1 <= n_c <= SAMPLE_MAX, temp > 0, 0 < top_p, the ranges of cp checked by the caller.  Called by EVERY thread of the workgroup on the
// device (lane = thread index, stride = workgroup size; the arguments and the arrays' contents are the same for all of them, so every branch is uniform and every thread
// meets the same barriers) and as lane 0 of 1 on the host.  The sequential sums are lane 0's; the order typical sampling needs is a counting placement, one lane per
// live candidate.  Scratch is the caller's (LDS on the device), SAMPLE_MAX entries each: sa, sb, L (the live list), ord.  p[0 .. n_c) = the probabilities (0 for a
// candidate outside L); *res is written by lane 0 and valid for every thread on return (a barrier closes the function).
MG4_SMP_HD inline void sample_chain(const float *v, int n_c, float temp, float top_p, const ChainParams &cp, uint32_t word, int lane, int stride, float *p, float *sa, float *sb,
                                    int *L, int *ord, ChainRes *res) {
    if (cp.mirostat == 2) {                                                  // llama_sample_token_mirostat_v2 behind top-k; the filters are ignored
        if (lane == 0) {
            const float mu = cp.mu != cp.mu ? smp::mul(2.0f, cp.tau) : cp.mu, w0 = smp::div(v[0], temp);
            float Z = 0.0f;
            for (int j = 0; j < n_c; j++) { sa[j] = expf(smp::sub(smp::div(v[j], temp), w0)); Z = smp::add(Z, sa[j]); }
            int n = n_c;
            for (int j = 0; j < n_c; j++) if (-log2f(smp::div(sa[j], Z)) > mu) { n = j; break; }
            if (n == 0) n = 1;
            float S = 0.0f;
            for (int j = 0; j < n; j++) S = smp::add(S, sa[j]);
            const int pick = chain_draw(sa, n, S, word);
            const float observed = -log2f(smp::div(sa[pick], S));
            for (int j = 0; j < n; j++) p[j] = smp::div(sa[j], S);
            for (int j = n; j < n_c; j++) p[j] = 0.0f;
            const unsigned long long mask = n >= 64 ? ~0ull : (1ull << n) - 1ull;
            res->pick = pick; res->kept = n; res->mask_lo = (unsigned)mask; res->mask_hi = (unsigned)(mask >> 32);
            res->mu = smp::sub(mu, smp::mul(cp.eta, smp::sub(observed, cp.tau))); res->observed = observed;
        }
        MG4_SMP_SYNC();
        return;
    }
    const bool typ = cp.typical_p < 1.0f;
    for (int j = lane; j < n_c; j += stride) { L[j] = j; ord[j] = j; }
    MG4_SMP_SYNC();
    if (lane == 0) {
        int m = n_c;
        if (cp.tfs_z < 1.0f && m > 2) {                                      // 1. tail-free (Sampler::tail_free, min_keep = 1): q, d1, d2 in place in sa
            const float A = chain_softmax(v, L, m, sa);
            for (int j = 0; j < m; j++) sa[j] = smp::div(sa[j], A);
            for (int i = 0; i < m - 1; i++) sa[i] = smp::sub(sa[i], sa[i + 1]);
            float s = 0.0f;
            for (int i = 0; i < m - 2; i++) { sa[i] = fabsf(smp::sub(sa[i], sa[i + 1])); s = smp::add(s, sa[i]); }
            const bool norm = s > 1e-6f;
            const float flat = smp::div(1.0f, (float)(m - 2));
            float c = 0.0f;
            int cut = m;
            for (int i = 0; i < m - 2; i++) { c = smp::add(c, norm ? smp::div(sa[i], s) : flat); if (c > cp.tfs_z && i >= 1) { cut = i; break; } }
            m = cut;
        }
        if (typ) {                                                           // 2. typical, its sequential half: q in sb, the typicality scores in sa
            const float A = chain_softmax(v, L, m, sb);
            float H = 0.0f;
            for (int j = 0; j < m; j++) { sb[j] = smp::div(sb[j], A); if (sb[j] != 0.0f) H = smp::add(H, smp::mul(-sb[j], logf(sb[j]))); }
            for (int j = 0; j < m; j++) sa[j] = sb[j] != 0.0f ? fabsf(smp::sub(-logf(sb[j]), H)) : INFINITY;
        }
        res->kept = m;
    }
    MG4_SMP_SYNC();
    const int m0 = res->kept;
    if (typ)                                                                 // the order by score ascending, equal scores by list position: ord[rank] = position
        for (int j = lane; j < m0; j += stride) {
            const float mine = sa[j];
            int rank = 0;
            for (int i = 0; i < m0; i++) rank += (sa[i] < mine || (sa[i] == mine && i < j)) ? 1 : 0;
            ord[rank] = j;
        }
    MG4_SMP_SYNC();
    if (lane == 0) {
        int m = m0;
        if (typ) {
            float c = 0.0f;
            int t = m;
            for (int i = 0; i < m; i++) { c = smp::add(c, sb[ord[i]]); if (c > cp.typical_p) { t = i + 1; break; } }
            if (t < m) {                                                     // the kept entries return to value order
                for (int j = 0; j < m; j++) p[j] = 0.0f;
                for (int i = 0; i < t; i++) p[ord[i]] = 1.0f;
                int mm = 0;
                for (int j = 0; j < m; j++) if (p[j] != 0.0f) L[mm++] = j;
                m = mm;
            }
        }
        if (top_p < 1.0f) {                                                  // 3. top-p
            const float A = chain_softmax(v, L, m, sa);
            float c = 0.0f;
            for (int j = 0; j < m; j++) { c = smp::add(c, smp::div(sa[j], A)); if (c >= top_p) { m = j + 1; break; } }
        }
        if (cp.min_p > 0.0f) {                                               // 4. min-p: a prefix, the first entry always in it
            const float A = chain_softmax(v, L, m, sa), thr = smp::mul(cp.min_p, smp::div(sa[0], A));
            for (int j = 1; j < m; j++) if (!(smp::div(sa[j], A) >= thr)) { m = j; break; }
        }
        const float w0 = smp::div(v[L[0]], temp);                            // 5. temperature, softmax, draw
        float S = 0.0f;
        for (int j = 0; j < m; j++) { sa[j] = expf(smp::sub(smp::div(v[L[j]], temp), w0)); S = smp::add(S, sa[j]); }
        const int at = chain_draw(sa, m, S, word);
        unsigned long long mask = 0;
        for (int j = 0; j < n_c; j++) p[j] = 0.0f;
        for (int j = 0; j < m; j++) { p[L[j]] = smp::div(sa[j], S); mask |= 1ull << L[j]; }
        res->pick = L[at]; res->kept = m; res->mask_lo = (unsigned)mask; res->mask_hi = (unsigned)(mask >> 32); res->mu = cp.mu; res->observed = 0.0f;
    }
    MG4_SMP_SYNC();
}

}  // namespace mg4
