// The three functions ggml keeps as fp16 tables -- exp, SiLU, GELU -- in ONE device definition each: gathered from the table (t != null) or, t == null, the table's VALUE
// computed.  Included by every kernel file that evaluates one (qtraits.hpp for the language model's kernels, vision_kernels.hip) and by the scalar test hook
// (test_hooks.cpp: minigpt4_amd_test_activation evaluates each over all 65 536 fp16 arguments; tests/test_gpu_activations.py pins the result to the oracle's tables).
#pragma once
#include "devutil.hpp"

namespace mg4 {

__device__ __forceinline__ float h2f_bits(unsigned short h) { return __half2float(__ushort_as_half(h)); }
__device__ __forceinline__ unsigned short f2h_bits(float f) { return __half_as_ushort(f2h_rn(f)); }
__device__ __forceinline__ float f16r(float f) { return __half2float(f2h_rn(f)); }
__device__ __forceinline__ float tab(const __half *t, float x) { return __half2float(t[f2h_bits(x)]); }
// Fast mode (round 5, SURVEY.md 9.5: "in fast mode evaluate in fp32"): the VALUE of ggml's fp16 tables computed instead of gathered -- table[x] = fp16(f(fp16(x))) with f
// evaluated in fp32 by the host libm; here f comes from the GPU's exp (v_exp_f32), so a result can differ from the table's by one fp16 ulp where f lands next to an fp16
// rounding boundary.  The contract, asserted on the device over every fp16 argument (tests/test_gpu_activations.py): every finite argument within ONE fp16 ulp of the table's
// entry, at most 63 of the 63 488 finite arguments different at all, +-0 / +-inf / NaN as the table has them.  Recorded on an MI355X
// (tests/golden/activation_deviation_observed.json): exp 0 arguments different, SiLU 2 (-0.7139, -2.725), GELU 1 (-0.3533), each by one ulp.
// A null table pointer selects the computed form.  Who passes null -- fast mode only; parity mode always gathers:
//   * exp:  the decode step's attention (Engine::tabs_dec_) and the ViT / Q-Former attention (Engine::tabs_vis_.exp); MINIGPT4_COMPUTED_TABLES=0 passes the tables again.
//           Prompt-row attention gathers;
//   * SiLU: (a) the decode step's stand-alone silu(h1) * h3 preparation launch (k_silu_mul_quant at one row, and the batched step's) -- the mat-vec's fused prologue and its
//           w1 | w3 pair epilogue always gather; (b) the F16 model's w1 | w3 pair launch (k_gemm_dma PAIR), which the engine uses for prompt chunks of 512 rows and more
//           (MINIGPT4_PAIR_SILU_COMPUTED=0: gathers).  SHORTER chunks of an F16 model and every quantised model's prompt pass gather: which arm a prompt row of an F16 model
//           sees depends on the size of the chunk it arrives in;
//   * GELU: the fused GEMM epilogues of the vision tower and the Q-Former (tabs_vis_.gelu; MINIGPT4_COMPUTED_GELU=0: gather); the stand-alone epilogue launch of vision files
//           with quantised Linear weights (k_lin_epilogue) always gathers.
__device__ __forceinline__ float exp_h(const __half *t, float x) { if (t) return tab(t, x); return f16r(__expf(f16r(x))); }
__device__ __forceinline__ float silu_h(const __half *t, float x) { if (t) return tab(t, x); const float xh = f16r(x); return f16r(xh / (1.0f + __expf(-xh))); }
// table[x] = fp16(0.5 x (1 + tanhf(u))), u = sqrt(2 / pi) x (1 + 0.044715 x^2).  The host's tanhf is accurately rounded and its 1 + tanhf then cancels for negative x; to land on
// the same fp32 value th must be tanh(u) rounded to fp32 BEFORE that sum.  tanh(|u|) = 1 - 2 / (exp(2 |u|) + 1) is: the small quantity 2 / (E + 1) keeps its relative accuracy
// and the subtraction from 1 only discards bits.  (The one-sided form 1 - 2 / (exp(2 u) + 1) is not: for u < 0 the sum exp(2 u) + 1 rounds away the low bits of a small
// exponential, th is off by ~2 fp32 ulp, and 1 + th multiplies that -- measured on the device: 423 of the fp16 arguments in [-5.16, -0.35] off the table, by up to 5 fp16 ulp.)
__device__ __forceinline__ float gelu_h(const __half *t, float x) {
    if (t) return tab(t, x);
    const float xh = f16r(x);
    const float u = 0.79788456080286535587989211986876f * xh * (1.0f + 0.044715f * xh * xh);
    const float th = copysignf(1.0f - 2.0f / (__expf(2.0f * fabsf(u)) + 1.0f), u);
    return f16r(0.5f * xh * (1.0f + th));
}

}  // namespace mg4
