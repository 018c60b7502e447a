// Row preparation of the decode step, defined once: rms_norm(x) * w | x as it is | silu(a) * b, then ggml's Q8_K / Q8_0 quantisation (quant_emit4, qtraits.hpp).
// Used by the standalone kernels (k_rms_quant, k_rms_quant_slabs) and by the mat-vec kernels that prepare their row(s) inside the launch (matvec_run, matvec_tn_run,
// k_matvec_ri).  Operand order and rounding are part of the results: every user must produce the same bits, so every step below exists in this file only.
// A piece is a function where every user compiles to the code it had with the piece written out, and preprocessor text where some kernel does not (tools/isa_diff.py);
// matvec_run still spells out row_total's loop and matvec_tn_run row_partial's two lines, for the same reason.
#pragma once
#include "qtraits.hpp"

namespace mg4 {

enum ProKind : int { PRO_NONE = 0, PRO_RMS = 1, PRO_PLAIN = 2, PRO_SILU = 3 };   // what a mat-vec launch does to its row first (PRO_SILU: the caller has applied silu to x)

// LDS image of ONE quantised row: the planes of an ActQ, back to back (only the planes the weight type reads are written).  F16 weights read the fp16 row, which the
// caller lays over the two int8 planes.  Launches add their own header in front: 128 bytes of partial sums (single row), 512 + TN images rounded to 16 (several rows).
__host__ __device__ constexpr size_t row_image_bytes(int K) { return (size_t)2 * K + (size_t)(K / 256 + 1) * 4 + (size_t)4 * (K / 32) * 4 + (size_t)(K / 16) * 2 + 64; }
__device__ __forceinline__ void row_image(ActQ &L, unsigned char *p, const int K) {
    L.q8k = reinterpret_cast<int8_t *>(p); p += (size_t)K;
    L.q80 = reinterpret_cast<int8_t *>(p); p += (size_t)K;
    L.dk = reinterpret_cast<float *>(p); p += (size_t)(K / 256 + 1) * 4;
    L.d0 = reinterpret_cast<float *>(p); p += (size_t)(K / 32) * 4;
    L.d1 = reinterpret_cast<float *>(p); p += (size_t)(K / 32) * 4;
    L.s1 = reinterpret_cast<float *>(p); p += (size_t)(K / 32) * 4;
    L.sum0 = reinterpret_cast<int *>(p); p += (size_t)(K / 32) * 4;
    L.bsk = reinterpret_cast<int16_t *>(p);
}

// ggml_rms_norm's sum: fp32 squares, added in double.  acc += the four squares of v, in element order.  (Text, not a function: behind a function boundary the
// mat-vec prologues compile to longer code.)
#define MG4_ROW_SUMSQ4(acc, v) do { acc += (double)((v).x * (v).x); acc += (double)((v).y * (v).y); acc += (double)((v).z * (v).z); acc += (double)((v).w * (v).w); } while (0)

// A thread's partial sum -> its wave's slot of red[]; after a workgroup barrier row_total adds the slots in wave order.
__device__ __forceinline__ void row_partial(double *red, double sum) {
    sum = wave_sum_d(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
}
__device__ __forceinline__ double row_total(const double *red, const int n_waves) {
    double tot = 0.0;
    for (int w = 0; w < n_waves; w++) tot += red[w];
    return tot;
}
__device__ __forceinline__ float row_mean(const double tot, const int K) { return (float)(tot / (double)K); }
__device__ __forceinline__ float row_scale(const float mean) { return 1.0f / sqrtf(mean + 1e-6f); }

// MINIGPT4_PARITY: the value of ggml_compute_forward_rms_norm's loop -- ONE double accumulator, element order -- without running 5120 dependent double additions on
// one lane (20 us per norm, 1.6 ms of a 13B token).  Every addend is >= 0, so the sequential sum S and the parallel sum `tot` both lie within K * 2^-53 (relative) of
// the exact sum; mean = (float)(S / K) is monotone in S, so if the two ends of tot (1 +- 4e-16 K: the two sums' errors and margin for the multiplications below)
// convert to the SAME float, that float is the oracle's mean, whatever S is.  Otherwise (a sum that close to a float rounding boundary: ~1e-4 of the rows) thread 0
// runs the literal loop.  Workgroup-uniform: every thread holds the same tot; red[0] (LDS) is overwritten.  (Text for matvec_run, whose parity kernels compile with
// their comparisons inverted around a function; k_rms_quant is the other way round and calls the function below.)
#define MG4_ROW_MEAN_ORACLE(mean, tot, K, row_, red) do { \
    const double delta_ = (double)(K) * 4e-16; \
    const float lo_ = (float)((tot) * (1.0 - delta_) / (double)(K)), hi_ = (float)((tot) * (1.0 + delta_) / (double)(K)); \
    mean = lo_; \
    if (lo_ != hi_) { \
        __syncthreads(); \
        if (threadIdx.x == 0) { double sq_ = 0.0; for (int i_ = 0; i_ < (K); i_++) sq_ += (double)((row_)[i_] * (row_)[i_]); (red)[0] = sq_; } \
        __syncthreads(); \
        mean = (float)((red)[0] / (double)(K)); \
    } \
} while (0)
__device__ __forceinline__ float row_mean_oracle(const double tot, const int K, const float *x, double *red) { float mean; MG4_ROW_MEAN_ORACLE(mean, tot, K, x, red); return mean; }

// The four prepared values of a thread, in front of quant_emit4.  y: the norm weight (PRO_RMS) or the second factor (PRO_SILU).
template <int KIND> __device__ __forceinline__ void row_value4(float v[4], const float4 x, const float4 y, const float scale) {
    if (KIND == PRO_RMS) { v[0] = (x.x * scale) * y.x; v[1] = (x.y * scale) * y.y; v[2] = (x.z * scale) * y.z; v[3] = (x.w * scale) * y.w; }
    else if (KIND == PRO_SILU) { v[0] = x.x * y.x; v[1] = x.y * y.y; v[2] = x.z * y.z; v[3] = x.w * y.w; }
    else { v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; }
}
// lanes past the end of the row loaded element 0 (clamped, unconditional loads): their values must not reach a block's maximum or sum
__device__ __forceinline__ void row_zero_unless(float v[4], const bool in_range) { if (!in_range) { v[0] = 0.0f; v[1] = 0.0f; v[2] = 0.0f; v[3] = 0.0f; } }

}  // namespace mg4
