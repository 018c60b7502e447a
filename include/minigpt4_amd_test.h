/*
 * minigpt4_amd_test.h -- entry points of libminigpt4_test.so ONLY (csrc/test_hooks.cpp + csrc/probe_kernels.hip linked with the product's objects).
 *
 * Single-kernel parity hooks, micro-benchmarks, hardware probes and host-only helpers for the CPU test tier.  None of these symbols is exported by the product
 * library libminigpt4.so (tests/test_cpu_host.py checks both export lists).  Plain C types only.
 */
#pragma once
#include "minigpt4_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

MINIGPT4_API int minigpt4_amd_copy_arenas(struct MiniGPT4Context *dst, struct MiniGPT4Context *src);   /* tests: device-to-device stand-in for the broadcast on one GPU */

/* ---- single-kernel hooks for parity tests (need a GPU; allocate + free their own device memory) ------------------ */
/* y[N][n_out] = W . x with ggml's quantised-activation arithmetic.  raw_w: the tensor bytes exactly as stored in a model file. */
MINIGPT4_API int minigpt4_amd_test_mul_mat(int ggml_type, const void *raw_w, int64_t n_in, int64_t n_out, const float *x, int64_t N, float *y);
/* the same through the parity-mode kernel (k_mul_mat_ref): the per-block fp32 terms in the CPU oracle's order -- results bit-identical to oracle/refcpu.c */
MINIGPT4_API int minigpt4_amd_test_mul_mat_ref(int ggml_type, const void *raw_w, int64_t n_in, int64_t n_out, const float *x, int64_t N, float *y);
/* prefill launch as the engine issues it for N > 4 rows: n_mat (1..3) equally shaped k-quant matrices (raw blocks back to back) against N rows in ONE launch of the LDS-staged
 * int8-MFMA kernels; residual ([n_mat][N][n_out]) optional; ks > 1 forces that K split (0 = the launcher's choice).  y: [n_mat][N][n_out].  4 = shape refused. */
/* prefill mat-mul micro-benchmark: n_mat random matrices [rows][cols] against N random rows, average microseconds per (set) launch; generation 2 = mmq2_kernels.hip, 1 = round-1 kernels */
MINIGPT4_API int minigpt4_amd_bench_mmq(int ggml_type, int rows, int cols, int n_mat, int N, int iters, int ks, int generation, float *us_per_launch);
MINIGPT4_API int minigpt4_amd_test_mmq2(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int64_t N, const float *residual, int ks, int generation, float *y);
/* The decode (N = 1) mat-vec launches as the engine issues them: n1 equally spaced matrices of type1 (raw1 = their file bytes back to back), optionally one more of
 * type2 in the same mixed-type launch; prep 1 = rms_norm(x) * x2, 2 = x, 3 = silu(x) * x2, run standalone (fuse = 0) or in the kernel prologue (fuse = 1);
 * epi = 1: y[g] = silu(W0[g] . a) * (W1[g] . a) (n1 == 2); epi = 2: every fp32 accumulation in the CPU oracle's order (k-quants; bit-identical to oracle/refcpu.c).  residual / y: (n1 + n2) * n_out floats.  Returns 4 when the shape is outside the kernel's range. */
MINIGPT4_API int minigpt4_amd_test_matvec(int type1, const void *raw1, int n1, int type2, const void *raw2, int n2, int64_t n_in, int64_t n_out, const float *x, const float *x2,
                                          int prep, int fuse, int epi, const float *residual, float *y);
/* the same with the SiLU arm chosen by the caller: silu_table = the table prep 3 / epi 1 gather from, or NULL = the computed arm (what the decode step's stand-alone
 * silu * mul preparation launch gets in fast mode: prep 3 with fuse 0; the fused prologue and the pair epilogue always gather, so NULL with them is refused: 1) */
MINIGPT4_API int minigpt4_amd_test_matvec_ex(int type1, const void *raw1, int n1, int type2, const void *raw2, int n2, int64_t n_in, int64_t n_out, const float *x, const float *x2,
                                             int prep, int fuse, int epi, const float *residual, const unsigned short *silu_table, float *y);
/* ONE launch of the decode mat-vec with the row preparation in its prologue (arguments as minigpt4_amd_test_matvec with fuse = 1), with or without the issue barrier: a
 * data-free barrier between the prologue's row loads and its first weight requests (built for the k-quants at K <= 6144; elsewhere the plain form runs).  y: the outputs
 * followed by `guard` floats that the launch must leave at their 0xFF fill.  Outputs do not depend on issue_barrier, bit for bit. */
MINIGPT4_API int minigpt4_amd_test_matvec_issue(int type1, const void *raw1, int n1, int type2, const void *raw2, int n2, int64_t n_in, int64_t n_out, const float *x, const float *x2,
                                                int prep, int epi, const float *residual, int issue_barrier, int guard, float *y);
MINIGPT4_API int minigpt4_amd_test_matvec_waves(void);   /* waves of a prologue launch that fills the device (wave w owns row groups w, w + waves, ...) */
/* The batched-decode mat-vec: N = 1..4 activation rows x[N][n_in] against n_mat (1..3) equally spaced matrices in one weight pass; y / residual: [n_mat][N][n_out].
 * Returns 4 when the shape / type is outside the kernel's range. */
MINIGPT4_API int minigpt4_amd_test_matvec_rows(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int N, const float *residual, float *y);
/* The same launch with the rows' preparation chosen: prepare = 0 -- a launch of its own in front (rms_w non-null: rms_norm(x_t) * rms_w there); prepare = 1 -- inside the
   mat-vec launch (rms_w non-null: the norm form, NULL: the rows as they are).  Returns 4 when the kernel has no such form for the type / n_in. */
MINIGPT4_API int minigpt4_amd_test_matvec_rows_prep(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int N, const float *residual,
                                                    const float *rms_w, int prepare, float *y);
/* The two-type launch of the batched decode (k_matvec_tn_mix; a "more bits" layer's wq | wk + wv): n_a equally shaped matrices of type_a (Q4_K / Q5_K) + n_b of type_b
 * (Q6_K), n_a + n_b <= 3, against N = 1..4 rows prepared by a launch of their own.  y: [n_a + n_b][N][n_out] and ONE GUARD ROW of n_out floats behind them, prefilled
 * with 0xFF bytes.  1 = bad arguments, 4 = the launcher refuses the types / shape (n_in above 6144) */
MINIGPT4_API int minigpt4_amd_test_matvec_rows_mixed(int type_a, const void *raw_a, int n_a, int type_b, const void *raw_b, int n_b, int64_t n_in, int64_t n_out, const float *x,
                                                     int N, float *y);
/* Host only: which in-launch preparations the decode mat-vec offers for (type, n_in).  bit 0: the single-row prologue (prep 1 / 2 / 3 of minigpt4_amd_test_matvec with
   fuse = 1), bit 1: the SiLU row-pair epilogue, bit 2: the multi-row prologue (prepare = 1 above).  -1: bad arguments. */
MINIGPT4_API int minigpt4_amd_test_matvec_predicates(int ggml_type, int64_t n_in);
/* Activation quantisation (optionally after rms_norm with weight w): returns Q8_K and Q8_0 images of x[N][K].
 * q8k: int8[N*K], dk: float[N*K/256], bsums: int16[N*K/16], q80: int8[N*K], d0: float[N*K/32] (fp16-rounded). Any may be NULL. */
MINIGPT4_API int minigpt4_amd_test_quantize(const float *x, const float *rms_w, int64_t N, int64_t K, int8_t *q8k, float *dk, int16_t *bsums, int8_t *q80, float *d0);
/* ---- the activation-preparation kernels and the consumers of a deferred split-K combine, one launch each (tests/test_gpu_act_prepare.py).  Common form: 1 = bad arguments,
 * before any device is looked for; 2 = no device; 3 = HIP error.  An ActQ's thirteen planes, a row of each in elements: q8k int8 [K], dk float [K / 256], bsk int16 [K / 16],
 * bsq int8 [K / 256 * 16], bs16 fp16 bits [K / 256 * 16], q16 fp16 bits [K], q80 int8 [K], d0 / d1 / s1 float [K / 32], sum0 int32 [K / 32], xh fp16 bits [K], xf float [K].
 * Every plane is device memory of N + 1 such rows prefilled with 0xFF bytes -- row N is a guard row -- and every non-NULL out pointer receives all N + 1 rows, so a plane
 * that `mask` does not select comes back as the fill.  mask: any OR of ACT_Q8K 1, ACT_Q80 2, ACT_F16 4, ACT_F32 8.  planes: which optional planes the ActQ carries --
 * 1 bsq, 2 bs16 (needs bsq), 4 q16; the others are always there. */
/* ONE launch_rms_quant (launcher 0: second = the norm weight [K], NULL = the rows as they are) or launch_silu_mul_quant (launcher 1: second = b [N][K], NULL = the rows as
 * they are; silu_table = the 65536 fp16 bit patterns gathered from, NULL = the computed arm) on x [N][K].  sequential_sum: launcher 0's one-thread sum of squares.
 * Refused: NULL x, N < 1, K < 4, K % 4, K % 256 with ACT_Q8K, K % 32 with ACT_Q80, a mask outside 1 .. 15, planes outside 0 .. 7 or bs16 without bsq, launcher not 0 / 1 */
MINIGPT4_API int minigpt4_amd_test_prepare(int launcher, const float *x, const float *second, int64_t N, int64_t K, int mask, int planes, int sequential_sum,
                                           const unsigned short *silu_table, int8_t *q8k, float *dk, int16_t *bsk, int8_t *bsq, unsigned short *bs16, unsigned short *q16,
                                           int8_t *q80, float *d0, float *d1, float *s1, int32_t *sum0, unsigned short *xh, float *xf);
/* ONE launch_rms_quant_slabs (launcher 0: a SlabSrc of n = 1, slabs [ks][stride]; residual [N][K] or NULL; in_place != 0: the residual lives in the x_out buffer, as x_ does in
 * the engine; w [K] the norm weight; x_out [N + 1][K] = residual + slabs comes back with its guard row) or launch_silu_mul_quant_slabs (launcher 1: n = 2, slabs [2][ks][stride],
 * a = matrix 0's sum, b = matrix 1's; always gathers from silu_table; residual, w and x_out must be NULL).  Element (row, i) of a slab is at row * K + i; the caller fills
 * the padding behind N * K.  Refused: as above, and ks outside 2 .. 16, stride < N * K, stride % 4, launcher 0 without w or x_out, in_place without residual, launcher 1
 * without silu_table */
MINIGPT4_API int minigpt4_amd_test_prepare_slabs(int launcher, const float *slabs, int ks, int64_t stride, const float *residual, int in_place, const float *w, int64_t N, int64_t K,
                                                 int mask, int planes, const unsigned short *silu_table, float *x_out, int8_t *q8k, float *dk, int16_t *bsk, int8_t *bsq,
                                                 unsigned short *bs16, unsigned short *q16, int8_t *q80, float *d0, float *d1, float *s1, int32_t *sum0, unsigned short *xh,
                                                 float *xf);
/* ONE launch_slab_flush on a SlabSrc of n = 1 .. 3 matrices built from host data.  mks [n] = the matrices' slab counts; slabs = every matrix's slabs back to back
 * (matrix i: mks[i] x stride floats), a matrix with mks[i] == 1 contributes none.  mixed == 0 (k_mmq2_reduce_set): every count equal and >= 2.  mixed != 0 (one
 * launch_slab_reduce per split matrix; SlabSrc::ks = mks[0] >= 2): mks[i] == 1 means matrix i is already in place -- its contents are taken from row i of y and must come back
 * bit for bit.  residual [n][stride], row i added to matrix i when bit i of residual_mask is set (NULL with mask 0).  y [n + 1][stride]: in / out, device rows prefilled with
 * 0xFF bytes, row n is a guard row.  Refused: a NULL array, n outside 1 .. 3, a count outside 1 .. 16, stride < 4, stride % 4, residual_mask outside the n bits or without
 * residual */
MINIGPT4_API int minigpt4_amd_test_slab_flush(int n, int mixed, const int32_t *mks, const float *slabs, int64_t stride, const float *residual, int residual_mask, float *y);
/* ONE launch_rope_kv_slabs on N rows of ONE conversation at positions pos0 .. pos0 + N - 1, with a slab count per matrix: mks [3] for q | k | v, slabs laid out as for
 * minigpt4_amd_test_slab_flush with E = n_head * hd, element (row, i) at row * E + i.  mks[2] == 1: v is already in place -- v_in_place [N][E] is its buffer (SlabSrc::mbase[2] =
 * y[2]) and the slabs hold none for it; otherwise v_in_place must be NULL.  q_out [N + 1][E]: the rotated q, 0xFF-prefilled with a guard row; kc / vc [n_ctx][E] fp16 bit
 * patterns, zero where nothing was appended (what one side of minigpt4_amd_test_rope_kv_seg returns for one segment of slot 0).  Refused: a NULL array, n_head < 1, hd < 2 or
 * odd, N < 1, pos0 < 0, pos0 + N > n_ctx, a count outside 2 .. 16 for q | k or 1 .. 16 for v, stride < N * E, stride % 4, v_in_place given or missing against mks[2] */
MINIGPT4_API int minigpt4_amd_test_rope_kv_slabs(int n_head, int hd, int n_ctx, int N, int pos0, const int32_t *mks, const float *slabs, int64_t stride, const float *v_in_place,
                                                 float *q_out, uint16_t *kc, uint16_t *vc);
/* The embedding gather alone (k_get_rows: the per-element decoder of every weight type), ONE launch_get_rows.  raw_table: n_rows rows of K weights as a model file stores
 * them (Q3_K rows are re-encoded as Q6_K first, as the engine's load path does); tokens[N] in [-1, n_rows).  out [N + 1][K]: prefilled with 0xFF bytes, row N is a guard
 * row; a token of -1 leaves its row at the fill.  1 = bad arguments, before any device is touched (a NULL pointer, a token outside [-1, n_rows), a K that is not a whole
 * number of blocks, an unknown type); 2 = no device; 3 = HIP error */
MINIGPT4_API int minigpt4_amd_test_get_rows(int ggml_type, const void *raw_table, int n_rows, int64_t K, const int32_t *tokens, int N, float *out);
/* C[M][N] = A[M][K] . W[N][K]^T on the MFMA f16 path (inputs given as fp32, rounded to fp16 on the device) + optional bias/GELU */
MINIGPT4_API int minigpt4_amd_test_gemm_f16(const float *A, const float *W, const float *bias, int M, int N, int K, int gelu, float *C);
/* the same through the skinny-M kernel of the Q-Former (k_gemm_f16_skinny: N % 16 == 0, K % 32 == 0; 4 otherwise) */
MINIGPT4_API int minigpt4_amd_test_gemm_f16_skinny(const float *A, const float *W, const float *bias, int M, int N, int K, int gelu, float *C);

/* the same two with the arm chosen by the caller: gelu_table = the 65536 fp16 bit patterns the GELU epilogue gathers from, or NULL = the computed arm (Tables::gelu null, what the
 * engine's fast mode passes); skinny != 0: the skinny-M kernel */
MINIGPT4_API int minigpt4_amd_test_gemm_f16_ex(const float *A, const float *W, const float *bias, int M, int N, int K, int gelu, int skinny, const unsigned short *gelu_table, float *C);
/* ---- the image encoder's kernels between its GEMMs, one launch each (tests/test_gpu_vision_kernels.py).  Common form: 1 = bad arguments, before any device is touched;
 * 2 = no device; 3 = HIP error or a launcher's host-side throw (a row longer than 2048, more than 12 slabs, D % hd != 0); 4 = the launcher returned false.  Every output
 * buffer is prefilled with 0xFF bytes and has ONE GUARD ROW past `rows`, copied back with the rows; nothing is copied back unless the call returns 0. */
/* launch_layernorm (k_layernorm<3|6|8>): x [rows][n], w [n], b [n] or NULL; sequential_sums != 0: parity mode's one-thread sums.  out [rows + 1][n] fp32 and / or
 * out_h [rows + 1][n] fp16 bit patterns (either may be NULL, not both) */
MINIGPT4_API int minigpt4_amd_test_layernorm(const float *x, const float *w, const float *b, int rows, int n, int sequential_sums, float *out, unsigned short *out_h);
/* launch_splitk_reduce_ln (k_splitk_reduce_ln<2|4|8|12, 3|6|8>): slabs = n_slabs x slab_stride floats, row r of slab z at z * slab_stride + r * n (slab_stride >= rows * n; the
 * caller fills the padding); bias [n] / residual [rows][n] or NULL; in_place != 0: ONE device buffer serves as residual and x_out (needs both), as the ViT blocks call it;
 * ln_w NULL: no LayerNorm (then ln_b / ln_out / ln_out_h must be NULL too).  x_out / ln_out [rows + 1][n] fp32, ln_out_h [rows + 1][n] fp16 bit patterns */
MINIGPT4_API int minigpt4_amd_test_splitk_reduce_ln(const float *slabs, int n_slabs, int64_t slab_stride, const float *bias, const float *residual, int in_place, int rows, int n,
                                                    const float *ln_w, const float *ln_b, float *x_out, float *ln_out, unsigned short *ln_out_h);
/* The split-K forms of the fp16 GEMM: slab z = the raw fp32 partial product over slice z's k columns.  A [M][K], W [N][K] fp32, rounded to fp16 on the device.
 * skinny == 0: slices = gemm_split_slices(K, slices_wanted) as the engine computes it, then launch_gemm_f16_splitk (k_gemm_f16 64x64 tiles; from 384 / 640 rows the 128x128 /
 * 256x128 k_gemm_dma ring tiles); skinny != 0: launch_gemm_f16_skinny_splitk with slices_wanted as given (4, nothing launched, when it refuses).  slabs_out: room for
 * slices_wanted slabs of [M][N]; the first *slices_used_out are written.  minigpt4_amd_test_set_splitk_xcd / _set_gemm_arm apply */
MINIGPT4_API int minigpt4_amd_test_gemm_f16_splitk(const float *A, const float *W, int M, int N, int K, int slices_wanted, int skinny, float *slabs_out, int *slices_used_out);
/* launch_gemm_f16_head_major with N = 3 * D (the ViT's qkv projection).  out = 3 * D guard floats, then [3][D / hd][M][hd], then 3 * D guard floats: (M + 2) * 3 * D floats */
MINIGPT4_API int minigpt4_amd_test_gemm_f16_head_major(const float *A, const float *W, const float *bias, int M, int D, int hd, int K, float *out);
/* launch_im2col: image [batch][3][224][224] fp32 -> patches [batch * 256 + 1][ldp] fp16 bit patterns (ldp >= 588; batch <= 16) */
MINIGPT4_API int minigpt4_amd_test_im2col(const float *image, int batch, int ldp, unsigned short *patches);
/* launch_assemble_embeddings: cls [D], pe [batch * 256][D], pos [257][D] -> x [batch * 257 + 1][D] */
MINIGPT4_API int minigpt4_amd_test_assemble(const float *cls, const float *pe, const float *pos, int batch, int D, float *x);
/* launch_lin_epilogue: out = [residual +] gelu?(bias + y); y / residual [rows][n], bias [n]; gelu_table (65536 fp16 bit patterns) non-NULL = with the GELU step, gathered
 * from it (this launch always gathers).  out [rows + 1][n] fp32 and / or out_h [rows + 1][n] fp16 bit patterns */
MINIGPT4_API int minigpt4_amd_test_lin_epilogue(const float *y, const float *bias, const float *residual, const unsigned short *gelu_table, int rows, int n, float *out,
                                                unsigned short *out_h);
/* exp / SiLU / GELU exactly as the kernels' epilogues call them (csrc/activations.hpp), evaluated on all 65536 fp16 bit patterns -> out[65536] fp16 bit patterns.
 * which: 0 GELU, 1 SiLU, 2 exp; table (65536 fp16 bit patterns) is gathered from, NULL selects the computed form */
MINIGPT4_API int minigpt4_amd_test_activation(int which, const unsigned short *table, unsigned short *out);
/* The ViT / Q-Former attention kernel (launch_attn_f32) on host rows q [batch * nq][heads * hd], k / v [batch * nk][heads * hd], hd 88 or 64, nk <= 320.  head_major != 0: the rows
 * reach the kernel as [head][batch * rows][hd] with head strides (the ViT's layout); qt: query tiles per workgroup, 0 = the launcher's choice; exp_table: ggml's fp16 exp table or
 * NULL = computed exponentials.  out [batch * nq][heads * hd] fp32, out_h (may be NULL) the same as fp16 bit patterns */
MINIGPT4_API int minigpt4_amd_test_attn_f32(const float *q, const float *k, const float *v, int heads, int hd, int nq, int nk, int batch, float q_prescale, float score_div, int head_major,
                                            int qt, const unsigned short *exp_table, float *out, unsigned short *out_h);

/* Micro-benchmark of the image path's fp16 GEMM on synthetic operands (tools/timeline_gemm.py). flags: 1 GELU, 2 residual, 4 fp16 output too; variant 0 = the dispatcher
 * (launch_gemm_f16), 1 = the skinny-M kernel, 2 + (slices << 8) = split K + k_splitk_reduce_ln; n_sets weight matrices are cycled (no Infinity-Cache repeats) */
MINIGPT4_API int minigpt4_amd_bench_gemm_f16(int M, int N, int K, int flags, int variant, int iters, int n_sets, float *us_per_launch);
/* Micro-benchmark of the ViT / Q-Former attention kernel on synthetic rows (tools/timeline_attn.py) */
MINIGPT4_API int minigpt4_amd_bench_attn_f32(int heads, int hd, int nq, int nk, int iters, float *us_per_launch);
/* the same with `batch` images per launch, computed exponentials (the engine's fast mode) and `qt` query tiles per workgroup forced (0 = the launcher's choice); nq == nk */
MINIGPT4_API int minigpt4_amd_bench_attn_f32_b(int heads, int hd, int nq, int nk, int batch, int qt, int iters, float *us_per_launch);
/* query tiles per workgroup of the ViT / Q-Former attention kernel for every later launch of this process (0 = the launcher's choice); bit-identical results for every value */
MINIGPT4_API void minigpt4_amd_test_set_attn_qt(int qt);
/* the F16 feed-forward pair launch: out_h[N][n_out] = fp16(silu_table(w1 x) * (w3 x)) (uint16 bit patterns), w = w1 then w3 as fp16 [n_out][n_in]; 4 = shape outside the path */
MINIGPT4_API int minigpt4_amd_test_f16_silu_pair(const float *x, const void *w_f16, int64_t N, int64_t n_in, int64_t n_out, unsigned short *out_h, float *out_f);
/* the same with the SiLU arm chosen by the caller (silu_table or NULL = computed, as above) */
MINIGPT4_API int minigpt4_amd_test_f16_silu_pair_ex(const float *x, const void *w_f16, int64_t N, int64_t n_in, int64_t n_out, const unsigned short *silu_table, unsigned short *out_h, float *out_f);
/* the context shift's kernel (launch_kv_shift) on host fp16 caches k / v = [n_layer][n_ctx][n_embd] (uint16 bit patterns, shifted in place): rows [n_keep + n_discard, n_rows)
 * move down by n_discard, keys re-rotated by -n_discard positions with the engine's RoPE table.  ms (may be NULL): hipEvent time of the launch.  1 = bad arguments */
MINIGPT4_API int minigpt4_amd_test_kv_shift(int n_layer, int n_ctx, int n_embd, int n_head, int n_rows, int n_keep, int n_discard, uint16_t *k, uint16_t *v, float *ms);
/* the prefix copy's kernel (launch_kv_copy) on host fp16 caches k / v = [n_slot][n_layer][rows][n_embd] (uint16 bit patterns, changed in place): rows [0, n_rows) of every
 * layer of slot src go to the n_dst slots dst.  src_rows = 0: the source is that slot, as laid out; src_rows > 0: the source is a COMPACT copy [n_layer][src_rows][n_embd] of
 * the slot's first src_rows rows (the prefix store's layout), built on the device before the launch.  ms (may be NULL): hipEvent time of the launch.  k == v == NULL: timing only -- the caches are
 * device buffers of that shape (filled, never copied to or from the host), for shapes too large to move through the host (n_ctx = 2048 rows per layer).  1 = bad arguments
 * (a slot out of range, src among dst, only one of k / v NULL), 3 = the launcher refused the shape (text in minigpt4_amd_last_error) */
MINIGPT4_API int minigpt4_amd_test_kv_copy(int n_slot, int n_layer, int rows, int n_embd, int src, const int32_t *dst, int n_dst, int n_rows, int src_rows, uint16_t *k, uint16_t *v,
                                           float *ms);
/* the snapshot kernels alone (launch_kv_pack / launch_kv_unpack) on host fp16 caches k / v = [n_layer][n_ctx][n_embd] of ONE conversation (uint16 bit patterns) and a host
 * block [tensor K, V][n_layer][n][n_embd].  pack: block_out <- rows [r0, r0 + n), *sum_out <- the checksum the launch accumulated (the wrapping 64-bit sum of the block's
 * 32-bit words).  unpack: the block is scattered into rows [r0, r0 + n) of k / v IN PLACE, *sum_out <- the checksum of what the launch read.  ms (may be NULL): hipEvent
 * time of the launcher's work in the stream: the 8-byte hipMemsetAsync that zeroes the checksum word, then the kernel.  k == v == block == NULL: timing only -- device buffers of that shape, filled, never copied to or from the host.  1 = bad arguments (only some of the
 * arrays NULL, n < 0, n > n_ctx), 3 = the launcher refused the shape (n_embd % 8, r0 < 0, r0 + n > n_ctx; text in
 * minigpt4_amd_last_error) */
/* k_checksum alone (device_checksum: the sum of the 32-bit words of [device_ptr, device_ptr + bytes), bytes rounded down to 4, mod 2^64) over any range the device can
 * read, pinned host memory included.  ms (may be NULL): hipEvent time around the call.  1 = bad arguments (NULL, a pointer that is not 4-byte aligned) */
MINIGPT4_API int minigpt4_amd_test_checksum(const void *device_ptr, size_t bytes, uint64_t *sum_out, float *ms);
MINIGPT4_API int minigpt4_amd_test_kv_pack(int n_layer, int n_ctx, int n_embd, int r0, int n, const uint16_t *k, const uint16_t *v, uint16_t *block_out, uint64_t *sum_out, float *ms);
MINIGPT4_API int minigpt4_amd_test_kv_unpack(int n_layer, int n_ctx, int n_embd, int r0, int n, const uint16_t *block, uint16_t *k, uint16_t *v, uint64_t *sum_out, float *ms);
/* the scoring kernel (launch_logprob_rows) on host logits [rows][ld] fp32 (ld >= n_vocab; only the first n_vocab floats of a row are read): per row the log-softmax of
 * targets[r] (-1: none, logprob 0), the first argmax and its log-softmax.  One launch; ms (may be NULL): its hipEvent time.  1 = bad arguments, before any device is
 * touched (a NULL pointer, rows < 1, n_vocab < 1, ld < n_vocab, a target >= n_vocab or < -1) */
MINIGPT4_API int minigpt4_amd_test_logprob_rows(const float *logits, int rows, int n_vocab, int ld, const int32_t *targets, float *logprob_out, int32_t *greedy_out,
                                                float *greedy_logprob_out, float *ms_out);
/* the top-N kernel (launch_topn_rows) on host logits [buf_rows][ld] fp32 (ld >= n_vocab; only the first n_vocab floats of a row are read).  `rows` rows are evaluated:
 * row r is buffer row row_index[r] (duplicates allowed), or r when row_index is NULL.  Per row: ids_out / logprobs_out [rows][top_n] = the first top_n tokens in the
 * order "logit descending, equal logits by ascending id" and their log-softmax (the bits minigpt4_amd_test_logprob_rows reports for them), rank_out = the number of tokens
 * that sort before targets[r] (-1: no target, rank -1), target_logprob_out = the target's log-softmax (0 without one).  One launch; ms_out (may be NULL): its hipEvent
 * time.  1 = bad arguments, before any device is touched (a NULL pointer other than row_index / ms_out, rows < 1, buf_rows < 1, n_vocab < 1, ld < n_vocab, top_n outside
 * 1..64 or above n_vocab, a target >= n_vocab or < -1, a row_index entry outside [0, buf_rows), rows > buf_rows without row_index) */
MINIGPT4_API int minigpt4_amd_test_topn_rows(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *row_index, int rows, int top_n, const int32_t *targets,
                                             int32_t *ids_out, float *logprobs_out, int32_t *rank_out, float *target_logprob_out, float *ms_out);
/* Beam search (minigpt4_amd.h states the rule).  A step's decision is 44 int32 words: parent[8], tok[8], score[8] (fp32 bit patterns), n_live, n_fin, fin_beam[8],
 * fin_score[8] (raw scores, fp32 bit patterns), two words of padding.  Candidates are [n_beams][2 n_beams], row i = what beam i lists, in k_topn_rows' order.
 * minigpt4_amd_test_beam_select_host, no GPU: a whole search over GIVEN candidates -- ids / logprobs [n_steps][n_beams][2 n_beams], row (t, i) = what beam i lists in step t --
 * through the rule's host function and the engine's book-keeping, the source at `position`.  scores0 / live0: the first step's beam scores and live mask (scores0 NULL: the
 * search's own first step -- beam 0 at score 0, the others dead).  It ends like the engine's search: when the finished list reaches n_beams, or after n_steps.  steps_out (may
 * be NULL): [steps run][44].  tokens_out [n_best][n_steps + 1] (-1 behind a row's length), lengths_out / scores_out [n_best], *n_out rows, stats[4] as minigpt4_amd_beam_search.
 * 1 = bad arguments (a NULL pointer other than scores0 / steps_out, n_beams outside 2 .. 8, n_steps < 1, n_best outside 1 .. n_beams, a length_penalty that is not finite, no live
 * beam, a step that cannot fill n_beams live beams).
 * minigpt4_amd_test_beam_select: the kernel (launch_beam_select, one launch) on one step's candidates; scores[n_beams] is replaced by the next step's, step_out[44] the result
 * block, row_tok_out[n_beams] the row tokens it wrote for the weight pass.  1 = bad arguments, 2 = no device, 3 = device error.
 * minigpt4_amd_test_kv_permute: the beam reordering kernel (launch_kv_permute, one launch) on host fp16 caches k / v = [n_slot][n_layer][n_ctx][n_embd] (uint16 bit patterns,
 * changed in place): rows [r0, r1) of every layer of the listed conversation slots[i] become what slots[parent[i]] held, i < n.  ms (may be NULL): hipEvent time of the launch.
 * k == v == NULL: timing only, on device buffers of that shape.  1 = bad arguments (n outside 2 .. 8, a slot out of range or listed twice, a parent outside [0, n), rows outside
 * the cache, only one of k / v NULL), 2 = no device, 3 = the launcher refused the shape (text in minigpt4_amd_last_error) */
MINIGPT4_API int minigpt4_amd_test_beam_select_host(int n_beams, int n_steps, const int32_t *ids, const float *logprobs, const float *scores0, uint32_t live0, int eos, int position,
                                                    float length_penalty, int n_best, int32_t *steps_out, int32_t *tokens_out, int32_t *lengths_out, float *scores_out,
                                                    int32_t *n_out, int32_t *stats);
MINIGPT4_API int minigpt4_amd_test_beam_select(int n_beams, const int32_t *ids, const float *logprobs, float *scores, uint32_t live, int eos, int n_vocab, int32_t *step_out,
                                               int32_t *row_tok_out);
MINIGPT4_API int minigpt4_amd_test_kv_permute(int n_slot, int n_layer, int n_ctx, int n_embd, const int32_t *slots, int n, const int32_t *parent, int r0, int r1, uint16_t *k,
                                              uint16_t *v, float *ms);
/* Penalties and logit bias (minigpt4_amd.h).  A table is [n][4] int32 words per entry: id, count, the bias's fp32 bit pattern, has_bias (0 / 1).
 * minigpt4_amd_test_penalise_host, no GPU: builds the table for `history` (row-aligned ids, -1 = embedding row) and the bias pairs (distinct ids in [0, n_vocab), at most
 * 256) with the engine's builder, applies it to row[n_vocab] in place with the host function, and writes the table to table_out (may be NULL; table_cap entries at
 * most) and the builder's flags (1 = repetition step runs, 2 = frequency / presence step runs, 4 = the newline id is exempt) to flags_out (may be NULL).  Returns the
 * number of table entries, or -1 on bad arguments.
 * minigpt4_amd_test_pen_pick: the kernel (launch_pen_pick, one launch, one workgroup per row) on host logits [buf_rows][ld] fp32 (only the first n_vocab floats of a row
 * are read).  rows = [n_rows][8] words: buffer row, first table entry, entries, flags, repeat_penalty / alpha_frequency / alpha_presence bit patterns, 0.  picked_out[n_rows]
 * = the first maximum of each transformed row, adjusted_out[n_table] (may be NULL) = the transformed value of every table entry.  1 = bad arguments, before any device is
 * touched (a NULL pointer, shapes < 1, ld < n_vocab, a row / table range / id out of range, duplicate ids within one row's table); 2 = no device; 3 = device error */
MINIGPT4_API int minigpt4_amd_test_penalise_host(float *row, int n_vocab, const int32_t *history, int n_history, int n_ctx, int32_t repeat_last_n, float repeat_penalty,
                                                 float alpha_presence, float alpha_frequency, int penalize_nl, const int32_t *bias_ids, const float *bias, int n_bias,
                                                 int32_t *table_out, int table_cap, int32_t *flags_out);
MINIGPT4_API int minigpt4_amd_test_pen_pick(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *rows, int n_rows, const int32_t *table, int n_table,
                                            int32_t *picked_out, float *adjusted_out, float *ms_out);
/* Guided decoding (minigpt4_amd.h states the rule): the kernel (launch_guide_rows, one launch, one workgroup per pair) on host logits [buf_rows][ld] fp32 (only the first
 * n_vocab floats of a row are read).  pairs = [n][2] buffer rows (guided row, guidance row; the two may be equal, a row may serve several pairs), scales[n], row_tok_index =
 * [n][2] indices into a 64-entry row-token array, -1 = the pair writes none.  row_tok_io[64]: the array's contents before the launch, replaced by its contents afterwards.
 * mixed_out (may be NULL): [n][n_vocab] guided rows; pick_out / pick_value_out [n]: each row's first maximum and its value.  ms_out (may be NULL): the launch's hipEvent
 * time.  1 = bad arguments, before any device is looked for (a NULL pointer other than mixed_out / ms_out, buf_rows < 1, n_vocab < 1, ld < n_vocab, n outside 1 .. 32, a
 * buffer row outside [0, buf_rows), a row-token index outside [-1, 64)); 2 = no device; 3 = device error */
MINIGPT4_API int minigpt4_amd_test_guide_rows(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *pairs, const float *scales, const int32_t *row_tok_index,
                                              int n, float *mixed_out, int32_t *pick_out, float *pick_value_out, int32_t *row_tok_io, float *ms_out);
/* Constrained decoding (minigpt4_amd.h states the pattern language and the rules).
 * minigpt4_amd_test_constraint_compile, no GPU: the compiler alone.  n_bytes = -1: strlen.  trans_out (may be NULL) receives [n_states][256] entries when cap_states >=
 * n_states, accept_out (may be NULL) the accepting bitmap, 32 words; *n_states_out = the automaton's states (0 = dead, 1 = start).  0; 1 = refused, the compiler's text in
 * err (may be NULL; err_cap bytes); -1 = bad arguments.
 * minigpt4_amd_test_constrain_index: k_constrain_index alone (one launch, one workgroup per state) on a GIVEN vocabulary -- vocab = the pieces' bytes back to back, off
 * [n_vocab + 1] where each begins -- and a given table trans [n_states][256] / accepting bitmap accept [(n_states + 31) / 32]; index_out [n_states][W], W = (n_vocab + 31)
 * / 32 rounded up to 4.  1 = bad arguments, before any device is touched (a NULL array, n_vocab < 1, n_states outside 2 .. 1024, offsets that do not start at 0 or
 * decrease, a table entry >= n_states); 2 = no device; 3 = device error.
 * minigpt4_amd_test_constrain_pick: k_constrain_pick alone (one launch, one workgroup per row) on host logits [buf_rows][ld].  rows / table as for
 * minigpt4_amd_test_pen_pick (entries 0 for a row without penalties); bitmaps = [n_bitmaps][W] allowed-id bitmaps, bitmap_of_row[n_rows] names each row's.  out[n_rows] =
 * the picked id, with bit 30 set when the row had no allowed id (the id is then 2).  1 = bad arguments as for _test_pen_pick, or a bitmap index out of range. */
MINIGPT4_API int minigpt4_amd_test_constraint_compile(const char *pattern, int n_bytes, uint16_t *trans_out, uint32_t *accept_out, int cap_states, int32_t *n_states_out,
                                                      char *err, size_t err_cap);
MINIGPT4_API int minigpt4_amd_test_constrain_index(const uint8_t *vocab, const int32_t *off, int n_vocab, const uint16_t *trans, const uint32_t *accept, int n_states,
                                                   uint32_t *index_out, float *ms_out);
MINIGPT4_API int minigpt4_amd_test_constrain_pick(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *rows, int n_rows, const int32_t *table, int n_table,
                                                  const uint32_t *bitmaps, int n_bitmaps, const int32_t *bitmap_of_row, int32_t *out, float *ms_out);
/* Device-side sampling (minigpt4_amd.h states the rule).
 * minigpt4_amd_test_philox, no GPU: Philox4x32-10 of counter[4] under key[2] -> out[4].  1 = a NULL pointer.
 * minigpt4_amd_test_sample_rule, no GPU: the rule's steps 1 to 4 on values[n_cand] (the candidates in order, 1 .. 64) with the given output word: returns the index of the
 * picked candidate, p_out[n_cand] = the probabilities (0 from kept on), *kept_out = kept.  -1 = bad arguments (a NULL pointer, n_cand outside 1 .. 64, temp not finite
 * or <= 0, top_p not > 0).
 * minigpt4_amd_test_sample_rows: k_sample_rows alone (one launch, one workgroup per row) on host logits [buf_rows][ld].  rows / table as for minigpt4_amd_test_pen_pick
 * (several rows may name one buffer row); bitmaps = [n_bitmaps][W] allowed-id bitmaps (may be NULL with n_bitmaps 0), bitmap_of_row[n_rows] names each row's, -1 = none;
 * temp_top_p = [n_rows][2]; top_k[n_rows]; seed_draws = [n_rows][2] 64-bit words; tok_index[n_rows] = an index into a 64-entry row-token array, -1 = the row writes none;
 * row_tok_io[64]: the array before the launch, replaced by its contents afterwards.  out = [n_rows][133] words: pick, stuck, the Philox word, n_cand, kept, 64 candidate
 * ids (-1 behind n_cand), 64 fp32 probabilities (0 behind kept).  ms_out (may be NULL): the launch's hipEvent time.  1 = bad arguments, before any device is looked for (as
 * for _test_pen_pick; a bitmap index outside [-1, n_bitmaps), a row-token index outside [-1, 64), top_k outside 1 .. min(64, n_vocab), temp not finite or <= 0, top_p
 * outside (0, 1]); 2 = no device; 3 = device error */
MINIGPT4_API int minigpt4_amd_test_philox(const uint32_t *counter, const uint32_t *key, uint32_t *out);
MINIGPT4_API int minigpt4_amd_test_sample_rule(const float *values, int n_cand, float temp, float top_p, uint32_t word, float *p_out, int32_t *kept_out);
MINIGPT4_API int minigpt4_amd_test_sample_rows(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *rows, int n_rows, const int32_t *table, int n_table,
                                               const uint32_t *bitmaps, int n_bitmaps, const int32_t *bitmap_of_row, const float *temp_top_p, const int32_t *top_k,
                                               const uint64_t *seed_draws, const int32_t *tok_index, int32_t *row_tok_io, int32_t *out, float *ms_out);
/* The extended rule of device-side sampling (minigpt4_amd.h states it): tail-free, typical, top-p, min-p, temperature, softmax and the draw, or mirostat v2.
 * minigpt4_amd_test_sample_chain, no GPU: the host side of the chain on values[n_cand] (the candidates in order, 1 .. 64) with the given output word and mu (NaN: unset):
 * returns the index of the picked candidate, p_out[n_cand] = the probabilities (0 for a candidate outside the live list), *kept_out = the live list's length, *mask_out =
 * bit j set when candidate j is in it, *mu_out = mu' (mirostat 0: mu as given), *observed_out = the observed surprise (mirostat 0: 0).  -1 = bad arguments (as
 * _test_sample_rule; tfs_z or typical_p outside (0, 1], min_p outside [0, 1], mirostat not 0 or 2, tau not finite or <= 0, eta not finite or < 0, an infinite mu).
 * minigpt4_amd_test_sample_rows_ex: k_sample_rows_ex alone; the arguments of _test_sample_rows, then chain = [n_rows][6] (tfs_z, typical_p, min_p, tau, eta, mu) and
 * mirostat[n_rows].  out = [n_rows][137] words: the 133 of _test_sample_rows (kept = the live list's length), the mask's low and high word, mu', the observed surprise.
 * Return codes as _test_sample_rows; 1 also for a chain parameter outside the ranges above. */
MINIGPT4_API int minigpt4_amd_test_sample_chain(const float *values, int n_cand, float temp, float top_p, float tfs_z, float typical_p, float min_p, int mirostat, float tau,
                                                float eta, float mu, uint32_t word, float *p_out, int32_t *kept_out, uint64_t *mask_out, float *mu_out, float *observed_out);
MINIGPT4_API int minigpt4_amd_test_sample_rows_ex(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *rows, int n_rows, const int32_t *table, int n_table,
                                                  const uint32_t *bitmaps, int n_bitmaps, const int32_t *bitmap_of_row, const float *temp_top_p, const int32_t *top_k,
                                                  const uint64_t *seed_draws, const int32_t *tok_index, const float *chain, const int32_t *mirostat, int32_t *row_tok_io,
                                                  int32_t *out, float *ms_out);
/* Speculation under sampling (minigpt4_amd.h states the rule).
 * minigpt4_amd_test_draft_sample: the sampled verify pass's epilogue alone -- k_sample_rows over the R rows (1 .. 8) of host logits [R][ld], then k_draft_sample_finish.
 * rows / table / bitmaps / bitmap_of_row / temp_top_p / top_k / seed_draws as for minigpt4_amd_test_sample_rows, one descriptor per row, descriptor r naming buffer row r;
 * row_tok[R] = the pass's row tokens (row_tok[0] is not compared); slot (0 or 1) = the conversation the pass belongs to; state_io = [2][3] (n_past, argmax, feed) of two
 * slots and slot_logits_io = [2][n_vocab] their logits rows, both replaced by their contents afterwards.  res_out[17] = {m, 8 picks, 8 stuck flags} (-1 behind R);
 * out = [R][133] words as for _test_sample_rows; ms_out (may be NULL): the hipEvent time of k_draft_sample_finish alone.  1 = bad arguments, before any device is looked
 * for; 2 = no device; 3 = device error.
 * minigpt4_amd_test_draft_tables, no GPU: the host staging of that pass (csrc/draft_host.hpp) for a history, x0 and a draft of at most 7 tokens (already cut for room).
 * trans / accept / n_states / state / vocab / off[n_vocab + 1] describe the constraint and the pieces (trans NULL: no constraint).  *n_rows_out = R, *cut_out = draft
 * tokens the constraint cut, rows_out = [R][8] words (PenRow: row, first entry, entries, flags, the three factors, 0), table_out = the R tables back to back
 * ([*n_table_out][4]: id, count, bias bits, has_bias), states_out[R] = q_r.  1 = bad arguments; 4 = table_cap too small (*n_table_out says what is needed). */
MINIGPT4_API int minigpt4_amd_test_draft_sample(const float *logits, int R, int n_vocab, int ld, const int32_t *rows, const int32_t *table, int n_table, const uint32_t *bitmaps,
                                                int n_bitmaps, const int32_t *bitmap_of_row, const float *temp_top_p, const int32_t *top_k, const uint64_t *seed_draws,
                                                const int32_t *row_tok, int slot, int32_t *state_io, float *slot_logits_io, int32_t *res_out, int32_t *out, float *ms_out);
MINIGPT4_API int minigpt4_amd_test_draft_tables(const int32_t *hist, int n_hist, int32_t x0, const int32_t *draft, int n_draft, int32_t repeat_last_n, float repeat_penalty,
                                                float alpha_presence, float alpha_frequency, int penalize_nl, const int32_t *bias_id, const float *bias_val, int n_bias, int n_ctx,
                                                int n_vocab, const uint16_t *trans, const uint32_t *accept, int n_states, int state, const uint8_t *vocab, const int32_t *off,
                                                int32_t *n_rows_out, int32_t *cut_out, int32_t *rows_out, int32_t *table_out, int table_cap, int32_t *n_table_out,
                                                int32_t *states_out);
/* Packed prompt rows of several conversations (minigpt4_amd_prefill_batch).  Caches kc / vc = [n_slots][n_ctx][n_head * hd] fp16 bit patterns, one layer per slot;
 * segs = [n_seg][3] (slot, rows, position of the first row), the segments' rows packed in that order in q = [N][n_head * hd] fp32.  Runs the segmented attention
 * (launch_attn_prefill_seg, one launch) into out_seg and one launch_attn_prefill per segment into out_ref.  form: 0 = the launchers' own choice, 1 = k_attn_prefill_h8,
 * 2 = k_attn_prefill_h QS 2, 3 = QS 1 (both sides), 4 = the exact-f32 kernel (both sides per segment).  *seg_launched = 1 when the one segmented launch ran.
 * out_h_seg / out_h_ref (both or neither; [N][E] fp16 bits): the launchers may store fp16 rows there instead (the F16 wo's input); wrote_h[0] / [1] = whether the
 * segmented side / every per-segment launch did.  The form applies to this call only.  1 = bad arguments */
MINIGPT4_API int minigpt4_amd_test_attn_prefill_seg(int n_head, int hd, int n_ctx, int n_slots, const uint16_t *kc, const uint16_t *vc, int n_seg, const int32_t *segs, const float *q,
                                                    int form, float *out_seg, float *out_ref, int *seg_launched, uint16_t *out_h_seg, uint16_t *out_h_ref, int *wrote_h);
/* RoPE + cache append of packed rows (k_rope_kv_seg; ks > 1: its slab form k_rope_kv_seg_slabs over ks copies of q | k | v) against k_rope_kv (_slabs) per segment.  segs as
 * above; q / k / v = [N][n_head * hd]; outputs: rotated q rows [N][E] and the caches [n_slots][n_ctx][E] (fp16 bits, zero where nothing was appended) of each side */
MINIGPT4_API int minigpt4_amd_test_rope_kv_seg(int n_head, int hd, int n_ctx, int n_slots, int n_seg, const int32_t *segs, const float *q, const float *k, const float *v, int ks,
                                               float *q_seg, uint16_t *kc_seg, uint16_t *vc_seg, float *q_ref, uint16_t *kc_ref, uint16_t *vc_ref);
/* Micro-benchmark of the prompt-row attention on a synthetic fp16 K / V cache (tools/timeline_attn_prefill.py); _timeline_attn: its stamps in a -DMG4_TIMELINE build */
MINIGPT4_API int minigpt4_amd_bench_attn_prefill(int n_head, int hd, int N, int n_past, int iters, float *us_per_launch);
MINIGPT4_API int minigpt4_amd_timeline_attn(unsigned long long *out, int max_workgroups);
/* force one tile shape (an "arm" of launch_gemm_f16_arm in vision_kernels.hip; 0 = the launcher's own choice) for every small-M GEMM / split-K GEMM
 * launched by the single-kernel hooks of this library, until set again (a context has its own tuning and never reads this one) */
MINIGPT4_API void minigpt4_amd_test_set_gemm_arm(int arm, int sk_arm);
/* 0: split-K GEMM slices in grid.z (the rounds 3-5 workgroup -> XCD mapping); 1 (default): the [slice][tile] work list dealt to the XCDs in contiguous ranges */
MINIGPT4_API void minigpt4_amd_test_set_splitk_xcd(int on);
/* Launch tuning (csrc/kernels.hpp: struct LaunchTuning) as n <= MINIGPT4_AMD_TUNING_FIELDS ints in the order cus, mv_waves_per_cu, mmq, mmqh, mmq_ks, mmq3_waves,
 * attn_prefill_w8, attn_prefill_f16, attn_prefill_form, gemm_arm, gemm_sk_arm, f16_ks, splitk_xcd, attn_vit_qt; both return the number of fields written (-1: bad arguments).
 * _tuning_from_env: what a context loaded now on a device with `cus` compute units would get (the defaults + MINIGPT4_ATTN_PREFILL_W8 / _MMQH / _ATTN_QT / _SPLITK_XCD /
 * _F16_KS; host only).  _context_tuning: what `ctx` got at its load */
#define MINIGPT4_AMD_TUNING_FIELDS 14
MINIGPT4_API int minigpt4_amd_test_tuning_from_env(int cus, int *out, int n);
MINIGPT4_API int minigpt4_amd_test_context_tuning(struct MiniGPT4Context *ctx, int *out, int n);
/* diagnostic builds (-DMG4_TIMELINE): the 32 clock stamps per workgroup of the last image-path GEMM launch; 0 = built without */
MINIGPT4_API int minigpt4_amd_timeline_vision(unsigned long long *out, int max_workgroups);
/* Micro-benchmark of the decode mat-vec kernels on synthetic weight planes (see bench_kernels.py). variant 0: one launch per matrix, 1: fused persistent-wave launch,
   2: the same with the rms-norm prologue, 3 / 4: the batched step's multi-row launch with 4 / 2 prepared rows, 5 / 6: 2 / 4 rows prepared inside the launch */
MINIGPT4_API int minigpt4_amd_bench_matvec(int ggml_type, int rows, int cols, int n_mat, int variant, int iters, int n_sets, int waves_per_cu, float *us_per_launch, double *bytes_per_launch);

/* Average latency (microseconds) of a device-wide barrier across n_blocks co-resident 512-thread workgroups (atomic counter + agent-scope fences); *errors
 * counts visibility failures of a neighbour-word check.  Measurement for DESIGN.md's launch-gap-vs-barrier analysis. */
/* batched decode on the int8 matrix cores (csrc/ri_kernels.hip): ordinary planes -> row-interleaved image -> N = 1..4 prepared rows against n_mat equally shaped Q4_K / Q5_K /
 * Q6_K matrices in one launch; y [n_mat][N][n_out]; returns 4 when the type / shape is outside the kernel's range */
MINIGPT4_API int minigpt4_amd_test_matvec_ri(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int N, const float *residual, const float *rms_w /* non-null: rows rms-normed with it inside the launch */, float *y);
MINIGPT4_API int minigpt4_amd_test_matvec_ri_mixed(int type_a, const void *raw_a, int n_a, int type_b, const void *raw_b, int n_b, int64_t n_in, int64_t n_out, const float *x, int N, float *y);   /* one launch over n_a matrices of Q4_K / Q5_K + n_b of Q6_K (a "more bits" layer's wq | wk + wv) */
MINIGPT4_API int minigpt4_amd_bench_matvec_ri(int ggml_type, int rows, int cols, int n_mat, int N, int iters, int n_sets, float *us_per_launch);   /* us per launch of the same, synthetic planes, rotating sets */
/* 1 when the test library was built by `make test-extras` (closed-direction kernels included: the generation-3 prompt mat-mul, the batched-decode MFMA probe), else 0 */
MINIGPT4_API int minigpt4_amd_test_extras(void);
MINIGPT4_API float minigpt4_amd_probe_grid_barrier(int n_blocks, int iters, unsigned *errors);
/* round 5 (csrc/tn_mfma_probe.hip, tools/batched_mfma_probe.py): the batched decode mat-vec on v_mfma_i32_4x4x4_16B_i8 over row-interleaved SYNTHETIC Q5_K planes -- microseconds per
 * launch for one rows x cols matrix set against TN = 1..4 prepared rows; check != 0 validates the launch against a scalar kernel over the same planes (relative difference out) */
MINIGPT4_API int minigpt4_amd_probe_tn_mfma(int rows, int cols, int TN, int iters, int n_sets, int check, float *us_per_launch, float *rel_diff);
/* what csrc/dist.cpp reads from MINIGPT4_WORLD_SIZE / MINIGPT4_RANK / MINIGPT4_NCCL_ID_FILE / MINIGPT4_DIST_TIMEOUT_S (host only): 0, or 1 with the reason in err */
MINIGPT4_API int minigpt4_amd_dist_env(int *world, int *rank, char *id_file, size_t cap, char *err, size_t err_cap);
/* LDS-DMA stream probe (csrc/probe_kernels.hip, tools/probe_dma.py): chip-wide GB/s of `waves` loader waves per CU keeping `depth` fills of `fill` bytes in flight into an LDS
 * ring; form 0 scalar base + instruction offsets, 1 per-lane addresses, 2 register loads, 3 register loads + ds_write; policy 0 nt, 1 default; deal 0 blocked, 1 round-robin */
MINIGPT4_API float minigpt4_amd_probe_dma(int form, int policy, int waves, int fill, int depth, int deal, double total_gb);
/* vector-ALU issue probe: ns per instruction and wave for one instruction kind (0 v_and, 1 v_dot4c_i32_i8, 2 v_mul_lo_u32, 3 v_mad_i32_i24, 4 v_fma_f32, 5 v_and_or,
   6 v_bfe_u32, 7 v_cvt_f32_i32, 8 v_dot4_i32_i8, 9 v_mad_u64_u32, 10 v_lshrrev) at 1..4 waves per SIMD; < 0 without a GPU */
MINIGPT4_API float minigpt4_amd_probe_valu(int op, int waves_per_simd, int iters);

/* The verify pass's attention launch alone (csrc/llm_kernels.hip k_attn_llm_draft).  q, k, v [R][n_head * hd] fp32 raw projections; kc, vc [n_slot][n_ctx][n_head * hd]
 * fp16 bit patterns, changed in place; the R rows belong to conversation `slot` at positions n_past .. n_past + R - 1; computed_exp != 0: the exponentials are computed
 * (what the engine's decode step gets by default), 0: gathered from the fp16 table.  mode 0: one launch_attn_llm_draft; mode 1: R one-row launches of the batched decode
 * attention kernel, the position advanced by one between them.  out [R][n_head * hd].  1 = refused before any device is touched (a NULL array, mode not 0 / 1, hd not
 * 32 / 64 / 128, n_head < 1, slot outside [0, n_slot), R outside 1 .. 8, n_past < 0, n_past + R > n_ctx, n_ctx above the kernel's LDS rows), 2 = no device, 3 = HIP error */
MINIGPT4_API int minigpt4_amd_test_attn_draft(int mode, int n_head, int hd, int n_ctx, int n_slot, int slot, int n_past, int R, int computed_exp, const float *q, const float *k,
                                              const float *v, uint16_t *kc, uint16_t *vc, float *out);
/* One launch of the decode attention body with `vs` workgroups per (head, row), each computing hd / vs of the head's output dims (csrc/llm_kernels.hip: VS; vs 1 is the
 * plain launch).  form 0: the one-row fused kernel (rows = 1, n_slot = 1, position n_past[0]); 1: the batched kernel, row r belongs to conversation row_slot[r] (all
 * different) at position n_past[row_slot[r]]; 2: the verify kernel, `rows` rows of conversation row_slot[0] at positions n_past[row_slot[0]] + r.  q, k, v [rows][n_head * hd]
 * fp32 raw projections; kc, vc [n_slot][n_ctx][n_head * hd] fp16 bit patterns, changed in place; row_slot [rows], n_past [n_slot]; computed_exp as above.
 * out [rows][n_head * hd].  1 = refused before any device is touched (a NULL array, form not 0 .. 2, hd not 32 / 64 / 128, vs not 1 / 2 / 4, n_head < 1, a slot outside
 * [0, n_slot) or used twice, rows outside 1 .. 8 for form 2 or not 1 for form 0, a position that leaves the cache, n_ctx above the kernel's LDS rows), 2 = no device,
 * 3 = HIP error */
MINIGPT4_API int minigpt4_amd_test_attn_vsplit(int form, int vs, int n_head, int hd, int n_ctx, int n_slot, int rows, const int32_t *row_slot, const int32_t *n_past,
                                               int computed_exp, const float *q, const float *k, const float *v, uint16_t *kc, uint16_t *vc, float *out);
/* The two attention paths that are otherwise reached only through a loaded model, on ONE conversation's caches kc, vc [n_ctx][n_head * hd] (fp16 bit patterns, changed in
 * place); q, k, v [rows][n_head * hd] fp32 raw projections; computed_exp as above.
 * mode 0: the key-split decode attention (launch_attn_llm_split: k_attn_split_scores + k_attn_split_pv, `splits` in 2 .. 16 workgroups per head) for `rows` successive
 * decode steps, step i on row i at position n_past + i, all on ONE workspace of attn_split_workspace_bytes bytes: filled with 0xFF bytes, its last 1 KiB + n_head words
 * zeroed ONCE before the first step (what the launcher asks of its caller), nothing between the steps.  q_rot is not used (may be NULL).
 * mode 1: the plain form of the decode attention (prompt rows beyond the prompt kernels' LDS rows): launch_rope_kv of the rows at positions n_past .. n_past + rows - 1,
 * then launch_attn_llm(fused = false); `splits` is ignored; q_rot [rows][E] receives the rotated q.
 * out [rows + 1][n_head * hd]: prefilled with 0xFF bytes, row `rows` is a guard row the launches must not touch.  1 = refused before any device is touched (a NULL array,
 * mode not 0 / 1, hd not 32 / 64 / 128, n_head outside 1 .. 64, rows outside 1 .. 64, n_past < 0, n_past + rows > n_ctx, n_ctx above the kernel's LDS rows, mode 0 with splits
 * outside 2 .. 16, mode 1 without q_rot), 2 = no device, 3 = HIP error */
MINIGPT4_API int minigpt4_amd_test_attn_rows(int mode, int n_head, int hd, int n_ctx, int n_past, int rows, int splits, int computed_exp, const float *q, const float *k,
                                             const float *v, uint16_t *kc, uint16_t *vc, float *q_rot, float *out);
/* ---- the greedy step epilogues alone (tests/test_gpu_step_epilogue.py): the kernels that end a decode step, a batched step, a packed prompt chunk and a greedy verify
 * pass, one launcher call each.  THE RULE all of them follow ("first maximum wins"): the id is the lowest index i with row[i] equal to the maximum over the row's
 * non-NaN entries, when that maximum is above -inf; otherwise (every entry NaN or -inf) it is 0.  A NaN is never chosen (`v > best` is false for it), -0.0 and +0.0
 * are equal (the lower index wins), and the 0x7FFFFFFF "nothing seen" index turns into id 0.  tests/greedy_ref.py: first_max.
 * Common form: 1 = bad arguments, before any device is looked for; 2 = no device; 3 = HIP error.  Every device output is prefilled with 0xFF bytes or holds what the
 * caller gave; every state array carries one guard word (logits: one guard row) behind its last slot, given by the caller and returned with the rest. */
/* ONE launch_argmax (k_argmax_part over 64 workgroups + k_argmax_final) on logits[n] with a 512-byte scratch, as the engine gives it.  *out = the id;
 * partial_values_out / partial_ids_out [64] (either may be NULL) = what each workgroup of the first launch left in the scratch (fp32 values; 0x7FFFFFFF = saw nothing).
 * Refused: NULL logits / out, n < 1, n > 2^24 */
MINIGPT4_API int minigpt4_amd_test_argmax(const float *logits, int n, int32_t *out, float *partial_values_out, int32_t *partial_ids_out);
/* form 0: ONE launch_batch_finish, row_slot_or_fin = row_slot[rows]; form 1: ONE launch_seg_finish, row_slot_or_fin = fin[rows][2] = (slot, new position).
 * logits [rows][n_vocab]; n_past_io / argmax_io / feed_io [n_slot + 1] words and slot_logits_io [n_slot + 1][n_vocab] are uploaded, and returned after the launch (the
 * last word / row is the guard).  Refused: a NULL array, form not 0 / 1, rows outside 1 .. 64, n_vocab outside 1 .. 2^20, n_slot outside rows .. 4096, a slot outside
 * [0, n_slot) or named twice */
MINIGPT4_API int minigpt4_amd_test_step_finish(int form, const float *logits, int rows, int n_vocab, int n_slot, const int32_t *row_slot_or_fin, int32_t *n_past_io,
                                               int32_t *argmax_io, int32_t *feed_io, float *slot_logits_io);
/* ONE launch_draft_finish (k_draft_argmax over the R rows, then k_draft_finish) on logits [R][n_vocab] with the pass's row tokens tok[R] (tok[0] is not compared) for
 * conversation `slot`.  State arrays as above.  res_out [1 + 8 + 1] words: m, the rows' ids, the 0xFF fill behind R, and a guard word behind the launcher's nine.
 * Refused: a NULL array, R outside 1 .. 8 (the launcher's own throw is never reached), n_vocab outside 1 .. 2^20, n_slot outside 1 .. 4096, slot outside [0, n_slot) */
MINIGPT4_API int minigpt4_amd_test_draft_finish(const float *logits, int R, int n_vocab, const int32_t *tok, int n_slot, int slot, int32_t *n_past_io, int32_t *argmax_io,
                                                int32_t *feed_io, float *slot_logits_io, int32_t *res_out);
/* The one-thread / one-wave bookkeeping launches on state arrays as above (all three are uploaded and returned, whichever the launch can reach).
 * form 0: ONE launch_advance(n_past + slot, n, with_tok0 ? feed + slot : NULL, argmax + slot), slot = row_slot[0]; row_pos is not used (may be NULL).
 * form 1: ONE launch_batch_begin(n_past, row_slot, row_pos, B = n), B in 1 .. 64, the slots distinct.
 * form 2: ONE launch_draft_begin(n_past, row_slot, row_pos): one slot, one position; n is not used.
 * Refused: a NULL array (row_pos: forms 1 / 2), form not 0 .. 2, n_slot outside 1 .. 4096, a slot outside [0, n_slot) or named twice, form 1 with n outside 1 .. 64 or
 * n > n_slot */
MINIGPT4_API int minigpt4_amd_test_step_words(int form, int n_slot, int n, const int32_t *row_slot, const int32_t *row_pos, int with_tok0, int32_t *n_past_io,
                                              int32_t *argmax_io, int32_t *feed_io);
/* ONE launch_gather_rows: dst[r] = src[idx[r]], rows of E floats, src [n_src][E], idx [n].  dst_out [n + 1][E]: prefilled with 0xFF bytes, row n is a guard row.
 * Refused: a NULL array, n_src / n outside 1 .. 65536, E outside 1 .. 2^20, an idx entry outside [0, n_src) */
MINIGPT4_API int minigpt4_amd_test_gather_rows(const float *src, int n_src, const int32_t *idx, int n, int E, float *dst_out);
/* ---- the verify pass of several conversations (minigpt4_amd_verify_draft_batch), its launches alone ---- */
/* The attention launch.  groups [n_groups][3] = (slot, p0, R): group g is R rows of conversation `slot` at positions p0 .. p0 + R - 1; the N = sum R <= 64 packed rows
 * follow in list order.  q, k, v, out [N][n_head * hd]; kc / vc [n_slot][n_ctx][n_head * hd] fp16 bit patterns, changed in place; vs 1 / 2 / 4 = the value-column split.
 * mode 0: launch_mdraft_begin on all-zero positions, then ONE launch_attn_llm_draft_batched.  mode 1: one launch_attn_llm_draft per group, in list order.
 * Otherwise as minigpt4_amd_test_attn_draft.  Refused (1, before a device is looked for): a NULL array, mode not 0 / 1, hd not 32 / 64 / 128, vs not 1 / 2 / 4,
 * n_head < 1, n_slot < 1, n_groups outside 1 .. 64, a slot outside [0, n_slot) or named twice, R outside 1 .. 8, p0 < 0 or p0 + R > n_ctx, more than 64 rows, n_ctx
 * beyond the verify form's LDS bound. */
MINIGPT4_API int minigpt4_amd_test_attn_draft_batch(int mode, int vs, int n_head, int hd, int n_ctx, int n_slot, int n_groups, const int32_t *groups, int computed_exp,
                                                    const float *q, const float *k, const float *v, uint16_t *kc, uint16_t *vc, float *out);
/* launch_mdraft_begin, then ONE launch_draft_finish_batch (k_draft_argmax over the N rows, then k_draft_finish_batch) on logits [N][n_vocab] with the pass's row tokens
 * tok[N], conversations row_slot[N] and positions row_pos[N].  State arrays as minigpt4_amd_test_step_finish's.  res_out [64 + 64 + 1] words: m per packed row (a
 * group's first row: its m; any other row: -1), the rows' greedy ids, 0xFF fill behind N in both halves, and a guard word.
 * Refused: a NULL array, N outside 1 .. 64, n_vocab outside 1 .. 2^20, n_slot outside 1 .. 4096, a slot outside [0, n_slot), rows of one slot that are not adjacent, a
 * group of more than 8 rows, positions that are negative or not consecutive inside a group. */
MINIGPT4_API int minigpt4_amd_test_draft_finish_batch(const float *logits, int N, int n_vocab, const int32_t *tok, const int32_t *row_slot, const int32_t *row_pos, int n_slot,
                                                      int32_t *n_past_io, int32_t *argmax_io, int32_t *feed_io, float *slot_logits_io, int32_t *res_out);

/* ---- host-only logic (no GPU needed) -------------------------------------------------------------------------------- */
/* the n-gram drafter of minigpt4_amd_decode_lookup alone (csrc/draft.cpp): the draft for a history of n tokens, at most n_draft tokens into out; returns its length
 * (0: no match), -1 for bad arguments (NULL history with n > 0, NULL out, n < 0, ngram_min < 1, ngram_max < ngram_min, n_draft < 0) */
MINIGPT4_API int minigpt4_amd_test_ngram_draft(const int32_t *history, int n, int ngram_max, int ngram_min, int n_draft, int32_t *out);
struct MiniGPT4Vocab;
MINIGPT4_API struct MiniGPT4Vocab *minigpt4_amd_vocab_load(const char *llm_path);            /* parses hparams + vocab of a GGJT v3 file */
MINIGPT4_API void minigpt4_amd_vocab_free(struct MiniGPT4Vocab *v);
MINIGPT4_API int minigpt4_amd_vocab_size(struct MiniGPT4Vocab *v);
MINIGPT4_API const char *minigpt4_amd_vocab_piece(struct MiniGPT4Vocab *v, int id, int *len);
MINIGPT4_API int minigpt4_amd_vocab_tokenize(struct MiniGPT4Vocab *v, const char *text, int add_bos, int32_t *out, int cap);
/* Parses both files without touching a GPU.  Returns a MiniGPT4Error; fills counts when non-NULL. */
MINIGPT4_API int minigpt4_amd_inspect_files(const char *vision_path, const char *llm_path, int *n_vision_tensors, int *n_llm_tensors, int64_t *llm_weight_bytes_per_token);
/* Pillow's 8-bit bicubic resample tables for in_size -> out_size (what the preprocess kernels consume): first/count: int[out_size],
 * kk: int[out_size * ksize] (22-bit fixed point).  Call with kk = NULL to learn ksize.  0, -1 (bad sizes) or -2 (kk_cap too small). */
MINIGPT4_API int minigpt4_amd_resample_coeffs(int in_size, int out_size, int *ksize, int *first, int *count, int *kk, size_t kk_cap);
/* Digest (FNV-1a 64) of what the engine takes from an LLM file -- hyper-parameters, vocabulary, every tensor's name / type / shape (and bytes when
 * with_data != 0).  GGJT v3 and GGUF v2 / v3 files of the same model digest equally.  Returns a MiniGPT4Error. */
MINIGPT4_API int minigpt4_amd_llm_file_digest(const char *llm_path, uint64_t *digest, int with_data);
/* ggml's reference block quantisers as minigpt4_quantize_model applies them (ggml_quantize_chunk): n floats (a whole number of blocks) -> dst; returns the
 * bytes written, 0 for an unsupported type (supported: Q4_0 Q4_1 Q5_0 Q5_1 Q8_0 Q4_K Q5_K Q6_K, ggml type ids) or a ragged n. */
MINIGPT4_API int64_t minigpt4_amd_quantize_chunk(int ggml_type, const float *x, void *dst, int64_t n);
/* Diagnostic builds only (-DMG4_TIMELINE): 8 x uint64 constant-clock (100 MHz) stamps per workgroup of the LAST decode mat-vec launch -- entry, first weight
 * request, activation row ready, first row group done, last row group done, results stored.  Returns the workgroups copied, 0 for a normal build, -1 on error. */
MINIGPT4_API int minigpt4_amd_timeline(unsigned long long *out, int max_workgroups);
/* The same builds: one further stamp per workgroup of that launch, taken when a prologue form has issued its row loads (in front of the first weight request). */
MINIGPT4_API int minigpt4_amd_timeline_rows(unsigned long long *out, int max_workgroups);
/* load-time re-encoding of Q3_K super-blocks (110 B) as value-identical Q6_K super-blocks (210 B); host only.  0 / 1 */
MINIGPT4_API int minigpt4_amd_convert_q3k_q6k(const void *src, void *dst, int64_t n_blocks);
/* Host sampler with an explicit seed (fresh std::mt19937 per call). */
MINIGPT4_API int minigpt4_amd_sample_logits(const float *logits, int n_vocab, int seed, float temp, int32_t top_k, float top_p, float tfs_z, float typical_p,
                                            int mirostat, float mirostat_tau, float mirostat_eta);

#ifdef __cplusplus
}
#endif
