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

}  // namespace mg4
