// Host-callable launchers of the gfx950 kernels (llm_kernels.hip, vision_kernels.hip).
#pragma once
#include <vector>

#include "common.hpp"
#include "penalty.hpp"
#include "beam.hpp"
#include "constraint.hpp"
#include "sampling.hpp"

namespace mg4 {

struct Tables {               // fp16 lookup tables, 65536 entries each, indexed by the fp16 bit pattern of the argument
    const __half *gelu = nullptr, *silu = nullptr, *exp = nullptr;
    int exp_neg_n = 0;         // entries of exp[0x8000 ...] (arguments -0, -2^-24, ...) up to and including the last nonzero finite one, rounded up to a multiple of 2048:
                               // the part of the table k_attn_vit keeps in LDS (softmax arguments are <= 0)
};

// ---- launch tuning -----------------------------------------------------------------------------------------------------
// Everything that decides a grid size, a kernel form or a K split besides the launch's own arguments.  A plain value: every context owns one (Engine::tune_, filled once
// at load), the test library's single-kernel hooks own another, and every launcher that reads a field takes it in front of its stream -- no process-global tuning state, so
// two contexts, or a context and a test hook, never change each other's launches.  What stays process-wide is measurement and logging only: the kernel-name tracing and
// launch probes, the timeline stamps of the diagnostic builds, the log verbosity, the thread-local last error, the launchers' function-local "attribute already set"
// flags and the CU count of probe_kernels.hip.
struct LaunchTuning {
    int cus = 256;               // compute units of the context's device (device properties)
    int mv_waves_per_cu = 0;     // decode mat-vec, prologue-free launches: waves per CU (0 = choose: 8; the mat-vec micro-benchmark sweeps it)
    int mmq = 2;                 // prompt rows (N >= 5): 2 = the LDS-staged int8-MFMA kernels of mmq2_kernels.hip, below 2 = v_dot4 tiles only (tests / A-B)
    int mmqh = 0;                // 1: Q4_K / Q5_K prompt rows on the fp16 matrix cores with the sub-block scales folded into the weight operands (k_mmqh_q45k; measured
                                 // slower, profiles/r05_prefill_fp16_scaled_operands.md; MINIGPT4_MMQH)
    int mmq_ks = 0;              // forced K split of launch_mmq2_set / launch_mmq3_set (0 = the launcher's choice)
    int mmq3_waves = 8;          // launch_mmq3_set: 8 = 128-row workgroups, one per CU; 4 = 64-row workgroups, two per CU (slower)
    int attn_prefill_w8 = 1;     // fp16 prompt attention: the 8-wave loader / MFMA form where its size rule selects it (MINIGPT4_ATTN_PREFILL_W8)
    int attn_prefill_f16 = 1;    // 1: prompt attention on the fp16 matrix cores, 0: the exact-f32 MFMA kernel
    int attn_prefill_form = 0;   // force one fp16 prompt attention form (1 = h8, 2 = h QS 2, 3 = h QS 1; 0 = the size rule)
    int gemm_arm = 0;            // force one tile shape for every small-M F16 GEMM (launch_gemm_f16_arm's arms); 0 = choose, -2 = the 64x64 launch always, -3 = round 2's
                                 // kernels everywhere (64x64 tiles, 128x128 large-M kernel)
    int gemm_sk_arm = 0;         // the same for the split-K GEMM (launch_gemm_f16_splitk_arm's arms); 0 = choose
    int f16_ks = 0;              // forced K split of the F16 language model's single-matrix prompt launches (wo, w2; 0 = choose, at most 8; MINIGPT4_F16_KS)
    int splitk_xcd = 1;          // 1: a split-K GEMM's work list [slice][tile] is dealt to the XCDs in contiguous ranges; 0: slices in grid.z (rounds 3-5; MINIGPT4_SPLITK_XCD)
    int attn_vit_qt = 0;         // query tiles per workgroup of k_attn_vit (0 = the launcher's choice; MINIGPT4_ATTN_QT)
    // the one place the fields' ranges are kept: the booleans 0 / 1, the forced counts >= 0, f16_ks <= 8, mmq3_waves 4 or 8, gemm_arm >= 0 or -2 or -3 (else the default)
    LaunchTuning normalised() const {
        LaunchTuning t = *this;
        t.mv_waves_per_cu = mv_waves_per_cu > 0 ? mv_waves_per_cu : 0; t.mmqh = mmqh != 0; t.mmq_ks = mmq_ks > 0 ? mmq_ks : 0; t.mmq3_waves = mmq3_waves == 4 ? 4 : 8;
        t.attn_prefill_w8 = attn_prefill_w8 != 0; t.attn_prefill_f16 = attn_prefill_f16 != 0; t.attn_prefill_form = attn_prefill_form >= 1 && attn_prefill_form <= 3 ? attn_prefill_form : 0;
        t.gemm_arm = gemm_arm >= 0 || gemm_arm == -2 || gemm_arm == -3 ? gemm_arm : 0; t.gemm_sk_arm = gemm_sk_arm > 0 ? gemm_sk_arm : 0;
        t.f16_ks = f16_ks < 0 ? 0 : f16_ks > 8 ? 8 : f16_ks; t.splitk_xcd = splitk_xcd != 0; t.attn_vit_qt = attn_vit_qt > 0 ? attn_vit_qt : 0;
        return t;
    }
};
// the tuning of a context on a device with `cus` compute units: the defaults + MINIGPT4_ATTN_PREFILL_W8, _MMQH, _ATTN_QT, _SPLITK_XCD, _F16_KS (engine.cpp; uses no device)
LaunchTuning launch_tuning_from_env(int cus);

// ---- load-time repack: raw ggml blocks (device copy of the file bytes) -> planes of a QWeight -------------------
// `dst` planes must already point into the arena (see plan_qweight).  raw/dst may not alias.
size_t plan_qweight(int type, int rows, int cols, QWeight &w, uint8_t *base);  // assigns plane pointers from `base`, returns bytes used
void launch_repack(const uint8_t *raw, const QWeight &w, hipStream_t s);
bool qweight_supported(int type);

// ---- activations -------------------------------------------------------------------------------------------------
// y = rms_norm(x) * w  (w == nullptr: y = x), quantised into the formats in `mask`; N rows of width K.
void launch_rms_quant(const float *x, const float *w, int N, int K, const ActQ &A, int mask, hipStream_t s, bool sequential_sum = false);   // sequential_sum: the sum of squares in element order by one thread (MINIGPT4_PARITY)
// y = silu(a) * b (fp16-table silu), quantised; or y = a when b == nullptr.
void launch_silu_mul_quant(const float *a, const float *b, int N, int K, const ActQ &A, int mask, const Tables &tb, hipStream_t s);

// ---- quantised mat-mul: y[t][r] = W[r] . act[t]  (+ residual[t][r]) ------------------------------------------------
void launch_mul_mat(const QWeight &W, const ActQ &A, int N, float *y, int ldy, const float *residual, const LaunchTuning &tune, hipStream_t s);

// MINIGPT4_PARITY=1: the same unit traits, the per-block fp32 terms added in the CPU oracle's order (one sequential chain per output) -- bit-identical to oracle/refcpu.c, slow
void launch_mul_mat_ref(const QWeight &W, const ActQ &A, int N, float *y, int ldy, const float *residual, const LaunchTuning &tune, hipStream_t s);
bool launch_mul_mat_ref_set(const QWeight *const *W, float *const *y, const float *const *res, int n, const ActQ &A, const LaunchTuning &tune, hipStream_t s);   // one row (decode) x 1..3 same-shape matrices: every unit of a row requested up front; false -> use launch_mul_mat_ref
bool matvec_prologue_supported(int type, int cols);   // the fused row-preparation variants of the decode mat-vec
// second-generation prefill kernels (mmq2_kernels.hip): 1..3 same-type, same-shape k-quant matrices against N >= 1 prepared rows (A.bsq required), weights streamed once per
// chunk of <= 128 tokens, activations staged through LDS, optional K split (partial sums in A.ws) combined in fixed order.  false -> outside the kernels' range, nothing launched.
bool mmq2_supported(int type, int rows, int cols);
// A split-K mat-mul whose combine step is left to its consumer (round 3): matrix m's ks slabs of `stride` floats start m * ks * stride floats into ws; the value of an
// element is (slab_0 + ... + slab_{ks-1}) (+ res[m]) and belongs at y[m].  ks <= 1: nothing pending.
struct SlabSrc { const float *ws = nullptr; int ks = 0; long long stride = 0; int n = 0; float *y[3] = {nullptr, nullptr, nullptr}; const float *res[3] = {nullptr, nullptr, nullptr};
                 // general form (results of TWO launches pending together, e.g. wq|wk and a differently typed wv): matrix m = sum of mks[m] slabs from mbase[m]; mks[m] == 1 with
                 // mbase[m] == y[m] is a matrix that is already in place.  Set by the deferring launches as mbase[m] = ws + m * ks * stride, mks[m] = ks.
                 const float *mbase[3] = {nullptr, nullptr, nullptr}; int mks[3] = {0, 0, 0}; bool mixed = false; };
void launch_slab_flush(const SlabSrc &src, hipStream_t s);                                      // the combine as its own launch (k_mmq2_reduce_set)
void launch_rms_quant_slabs(const SlabSrc &src, const float *w, int N, int K, const ActQ &A, int mask, hipStream_t s);       // n == 1: y[0] = res[0] + slabs, then rms norm * w, quantised
void launch_silu_mul_quant_slabs(const SlabSrc &src, int N, int K, const ActQ &A, int mask, const Tables &tb, hipStream_t s);   // n == 2: silu(a) * b, quantised
void launch_rope_kv_slabs(const SlabSrc &src, int N, int n_head, int hd, const int *n_past, const float *cos_tab, const float *sin_tab, __half *kcache, __half *vcache, hipStream_t s);   // n == 3
// defer != nullptr: with a K split the combine launch is skipped and *defer describes the slabs (ks > 1); otherwise *defer is cleared
bool launch_mmq2_set(const QWeight *const *W, float *const *y, const float *const *residual, int n, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s, SlabSrc *defer = nullptr,
                     int force_ks = 0);   // force_ks == 1: no K split = the CPU oracle's fp32 order (parity mode's prompt rows)
// (test library only: measured in round 4, not adopted) prompt mat-mul on load-time digit planes (mmq3_kernels.hip): Q4_K / Q5_K, sub-block scale x quant stored as 128 hi + lo (1.5 B per weight) in MFMA-fragment order
bool mmq3_supported(int type, int rows, int cols);
size_t mmq3_plane_bytes(int rows, int cols, size_t *hi_off = nullptr);
void launch_mmq3_build(const QWeight &W, uint8_t *planes, hipStream_t s);
bool launch_mmq3_set(const QWeight *const *W, const uint8_t *const *planes, float *const *y, const float *const *residual, int n, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s, SlabSrc *defer = nullptr);
int probe_tn_mfma(int rows, int cols, int TN, int iters, int n_sets, int check, int cus, float *us_per_launch, float *rel_diff);   // (test library with `make test-extras` only) tn_mfma_probe.hip
void launch_slab_reduce(const float *slabs, int n_slabs, long long slab_stride, const float *residual, float *y, size_t n, hipStream_t s);   // y = (residual +) sum_z slab_z, fixed order
// F16 weights at prompt sizes: 1..3 equally spaced [N][K] matrices x M fp16 rows in one launch of the 128x128 LDS-DMA GEMM (split K when the tiles do not fill the chip);
// false -> outside this path, nothing launched
bool launch_gemm_f16_silu_pair(const __half *A, int lda, const __half *W1, const __half *W3, int M, int N, int K, const Tables &tb, float *out, __half *out_h, int ldo, const LaunchTuning &tune, hipStream_t s);   // fp16(silu(A.W1^T) * (A.W3^T)) in one launch (F16 w1|w3 at prompt sizes)
bool launch_gemm_f16_set(const __half *A, int lda, const __half *const *W, int n, int M, int N, int K, float *const *y, const float *const *residual, int ldo, float *ws,
                         size_t ws_floats, const LaunchTuning &tune, hipStream_t s, SlabSrc *defer = nullptr);

// decode (N = 1) persistent-wave mat-vec over 1..3 same-type, same-shape matrices (wq|wk|wv, w1|w3); false -> caller falls back to launch_mul_mat
// pro: 0 = activations come from `A` (prepared by launch_rms_quant / launch_silu_mul_quant); 1 = rms_norm(px) * pw, 2 = px, 3 = silu(px) * pw are
// prepared and quantised inside the kernel prologue (one launch less per use).
// issue_bar (pro != 0): a data-free barrier between the prologue's row loads and its first weight requests, so that the row loads of all waves of a CU are issued first
// (built for the k-quants at K <= 6144; elsewhere the plain form runs).  Outputs do not depend on it, bit for bit.
bool launch_matvec_set(const QWeight *const *W, float *const *y, const float *const *residual, int n, const ActQ &A, const LaunchTuning &tune, hipStream_t s, int pro = 0, const float *px = nullptr,
                       const float *pw = nullptr, const Tables *tb = nullptr, int epi = 0, bool issue_bar = false);   // epi 1: y[0][g] = silu(W0[g].x) * (W1[g].x) (n == 2); MATVEC_EPI_REF: the CPU oracle's fp32 order (k-quants; pro 0..2)
constexpr int MATVEC_EPI_REF = 2;
int matvec_prologue_waves(const LaunchTuning &tune);   // waves of a prologue launch with at least as many row groups: wave w owns groups w, w + waves, ...
bool matvec_silu_pair_supported(int type, int cols);
// batched decode: N = 1..4 activation rows (prepared in `A`) against 1..3 same-type, same-shape, equally spaced matrices, weights streamed once;
// y[m][t * ldy + r] (+ residual[m][t * ldy + r]).  false -> outside the kernel's range, use launch_mul_mat.
bool launch_matvec_rows(const QWeight *const *W, float *const *y, const float *const *residual, int n, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s, const float *px = nullptr,
                        const float *pw = nullptr, int ldx = 0);   // px != null: rows t of x (stride ldx) are prepared inside the launch (A unused): pw != null rms-normed with pw, pw == null taken as they are; then quantised
bool matvec_rows_prologue_ok(int type, int K);
// batched decode on v_mfma_i32_4x4x4_16B_i8 over the row-interleaved image (ri_kernels.hip, round 5): N = 1..4 PREPARED rows (Q8_K image incl. bsk / bsq) against 1..3 same-type,
// same-shape Q4_K / Q5_K / Q6_K matrices; false -> outside the kernel's range, nothing launched
bool ri_supported(int type, int rows, int cols);
size_t ri_plan(int type, int rows, int cols, RiPlanes &p, uint8_t *base);      // assigns the image's plane pointers from `base` (nullptr: sizes only), returns the bytes used
void launch_ri_build(const QWeight &w, const RiPlanes &p, hipStream_t s);      // ordinary planes -> row-interleaved image
// workspace of the K-split form (few row groups, long K: the 13B w2): slabs for the workgroups' partial sums and one arrival ticket per row group, ZEROED by the owner (the kernel
// leaves them zero); without it (all null) such sets run one workgroup per group.  Owned by the caller -- one per context (Engine::ri_ws_), passed with every launch: no
// process-global state, so two contexts decoding on different threads / streams never share slabs or tickets (round-5 advisor).
struct RiWorkspace { float *slabs = nullptr; size_t slab_floats = 0; unsigned *tickets = nullptr; int n_tickets = 0; };
bool launch_matvec_ri(const QWeight *const *W, const RiPlanes *const *ri, float *const *y, const float *const *residual, int n, const ActQ &A, int N, int ldy, const LaunchTuning &tune,
                      hipStream_t s, const float *px = nullptr, const float *pw = nullptr, int ldx = 0, const RiWorkspace &ws = RiWorkspace{});   // px != null: rows t of px (stride ldx) are rms-normed with pw and quantised inside the launch (A unused)
// a "more bits" layer's set in one launch: na matrices of Q4_K / Q5_K + nb of Q6_K (na + nb <= 3), same shape, prepared rows
bool launch_matvec_ri_mixed(const QWeight *const *Wa, const RiPlanes *const *ria, float *const *ya, int na, const QWeight *const *Wb, const RiPlanes *const *rib, float *const *yb, int nb,
                            const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s);
int ri_ksplit(int total_groups, int K, const RiWorkspace &ws, const LaunchTuning &tune);   // workgroups per row group the launch would use with this workspace (1 = no K split)
// two k-quant types (Q4_K|Q5_K + Q6_K) with the same K in one launch; pro: 0 or 1 (rms_norm prologue)
bool launch_matvec_mixed(const QWeight *const *W1, float *const *y1, int n1, const QWeight *const *W2, float *const *y2, int n2, const ActQ &A, const LaunchTuning &tune, hipStream_t s, int pro = 0,
                         const float *px = nullptr, const float *pw = nullptr, int epi = 0, bool issue_bar = false);
// the same for N = 1..4 rows of the batched step (K <= 6144); px != null: rows rms-normed with pw and quantised inside the launch
bool launch_matvec_rows_mixed(const QWeight *const *W1, float *const *y1, int n1, const QWeight *const *W2, float *const *y2, int n2, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s,
                              const float *px = nullptr, const float *pw = nullptr, int ldx = 0);
// measurement: while tracing is on, every launcher of llm_kernels.hip notes the kernel symbol it launched (as rocprofv3 prints it, without the argument list)
void kernel_name_tracing(bool on);
const char *last_kernel_name();          // "" when nothing was launched since the last reset
void reset_kernel_name();
size_t launch_probe_count();                       // launches noted (and probed with their own start / stop events) since tracing was switched on
float launch_probe_us(size_t first, size_t last);  // sum of the dispatch durations of probes [first, last) in microseconds (stream synchronised); < 0: not available
int read_matvec_timeline_rows(unsigned long long *out, int max_workgroups);   // the same builds: one stamp per workgroup, taken when a prologue launch has issued its row loads
int read_matvec_timeline(unsigned long long *out, int max_workgroups);   // diagnostic builds (MG4_TIMELINE): stamps of the last decode mat-vec launch; 0 otherwise
int read_attn_timeline(unsigned long long *out, int max_workgroups);     // prompt attention (8 x u64 per workgroup, up to 2048 workgroups)
int read_vision_timeline(unsigned long long *out, int max_workgroups);   // the same for the image path's kernels (32 x u64 per workgroup)

// ---- token embedding gather (raw ggml rows, dequantised to f32) -----------------------------------------------------
void launch_get_rows(int type, const uint8_t *raw_table, int K, const int *tokens, int N, float *out, hipStream_t s);

// ---- RoPE + KV append, attention, argmax ----------------------------------------------------------------------------
// q,k,v: [N][E] f32.  Rotates q in place, writes rotated k and v as fp16 into the caches at position *n_past + t.
void launch_rope_kv(float *q, const float *k, const float *v, int N, int n_head, int hd, const int *n_past, const float *cos_tab,
                    const float *sin_tab, __half *kcache, __half *vcache, hipStream_t s);
// host: the RoPE tables every launch above reads, [n_ctx][hd / 2] fp32 cos / sin with ggml's iterative theta
void rope_tables(int n_ctx, int hd, std::vector<float> &cos_out, std::vector<float> &sin_out);
// context shift of ONE conversation: caches kc_slot / vc_slot = [n_layer][n_ctx][E] fp16.  Rows [n_keep + n_discard, n_rows) move to row - n_discard (in place, any
// overlap); moved keys are rotated by -n_discard positions with the table row cos / sin[n_discard], values copied bit for bit.  Rows below n_keep are not touched.
// Launches nothing when no row moves.
void launch_kv_shift(__half *kc_slot, __half *vc_slot, int n_layer, int n_ctx, int E, int hd, int n_keep, int n_discard, int n_rows, const float *cos_tab,
                     const float *sin_tab, hipStream_t s);
// prefix copy (Engine::fork, the prefix store): rows [0, n_rows) of every layer, keys and values, from ONE source (src_k / src_v = [n_layer][src_rows][E] fp16) to n_dst
// destinations (dst.k[d] / dst.v[d] = [n_layer][dst_rows][E]), bit for bit, in one launch; each 16-byte piece is loaded once and stored n_dst times.  Rows from n_rows on
// are not touched.  n_rows == 0 launches nothing.  Throws HipError: E % 8, n_rows above src_rows or dst_rows, n_dst outside 1..KV_COPY_MAX_DST, a destination region
// that overlaps the source's.
constexpr int KV_COPY_MAX_DST = 64;                    // = Engine::MAX_CONVERSATIONS
struct KvCopyDst { __half *k[KV_COPY_MAX_DST]; __half *v[KV_COPY_MAX_DST]; };   // passed by value to the kernel (llm_kernels.hip: why)
void launch_kv_copy(const __half *src_k, const __half *src_v, int src_rows, const KvCopyDst &dst, int n_dst, int dst_rows, int n_layer, int E, int n_rows, hipStream_t s);
// snapshot blocks (Engine::state_save / state_load): rows [r0, r0 + n) of every layer, keys and values, of ONE conversation (kc_slot / vc_slot = [n_layer][n_ctx][E] fp16)
// to / from one contiguous block [tensor K, V][layer][row][E] of 4 * n_layer * n * E bytes, bit for bit, in one launch.  *sum (device, 8-byte aligned; zeroed by the launcher
// in the stream) receives the block's checksum -- device_checksum's definition: the sum of its 32-bit words mod 2^64 --: of what pack wrote, of what unpack read.  Rows
// outside the range are not touched.  n == 0 launches nothing and leaves *sum 0.  Throws HipError: E % 8, a pointer that is not 16-byte aligned, r0 < 0, r0 + n > n_ctx,
// 2^31 or more 16-byte pieces.
void launch_kv_pack(const __half *kc_slot, const __half *vc_slot, int n_ctx, int n_layer, int E, int r0, int n, __half *block, unsigned long long *sum, hipStream_t s);
void launch_kv_unpack(const __half *block, __half *kc_slot, __half *vc_slot, int n_ctx, int n_layer, int E, int r0, int n, unsigned long long *sum, hipStream_t s);
// beam reordering (Engine::beam_search): rows [r0, r1) of every layer, keys and values, among W conversations of ONE cache pair (kc / vc = [slot][n_layer][n_ctx][E] fp16,
// conversation x at kc + x * seq_stride): conversation slots.s[i] receives what conversation slots.s[parent[i]] held, for ANY map parent[0 .. W) -- swaps, cycles,
// all-to-one -- in one launch; parent is read on the device (k_beam_select's output; an entry outside [0, W) counts as i).  An identity map returns at once; rows outside
// [r0, r1) and conversations not listed are not touched.  r0 == r1 launches nothing.  Throws HipError: W outside 2 .. KV_PERMUTE_MAX, E % 8, a region that is not 16-byte
// aligned, r0 < 0, r1 < r0, r1 > n_ctx, a slot outside [0, n_slots), duplicate slots, 2^31 or more 16-byte pieces.
constexpr int KV_PERMUTE_MAX = 8;                      // = BEAM_MAX
struct KvPermuteSlots { int s[KV_PERMUTE_MAX]; };      // passed by value to the kernel, as KvCopyDst is
void launch_kv_permute(__half *kc, __half *vc, size_t seq_stride, int n_slots, const KvPermuteSlots &slots, int W, const int *parent, int n_layer, int n_ctx, int E, int r0, int r1,
                       hipStream_t s);
// out[t][h*hd+i] = softmax(K q / sqrt(hd)) V over keys 0..*n_past+t.  caches: [n_ctx][E] fp16.
// fused (decode, N == 1): q,k,v are the raw projections; RoPE of q/k and the KV append happen inside the kernel.
// !fused: launch_rope_kv must have run (q rotated in place, caches appended).
// vs (this launcher, the batched and the verify one): 1, or 2 / 4 = that many workgroups per (head, row), each with its own hd / vs output dims (fused forms only; same
// bits out; attn_vsplit_ok says what is instantiated, the launchers throw for the rest).
bool attn_vsplit_ok(int hd, int vs);
void launch_attn_llm(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int N, int n_head, int hd, const int *n_past, int n_ctx,
                     const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, bool fused, hipStream_t s, int vs = 1);
// key-split decode attention for long contexts (one row; RoPE + KV append fused): every head's keys are shared by `splits` workgroups in two launches (scores; softmax + P.V
// + deterministic combine by the last-arriving workgroup of the head).  ws: attn_split_workspace_bytes() bytes of device memory whose LAST 1 KiB + n_head words (the arrival
// counters) were zeroed once; the kernels leave them zero.
size_t attn_split_workspace_bytes(int n_head, int hd, int n_ctx, int splits);
int attn_split_count(int n_head, int cus);
void launch_attn_llm_split(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int n_head, int hd, const int *n_past, int n_ctx, const float *cos_tab,
                           const float *sin_tab, const Tables &tb, float *out, void *ws, int splits, hipStream_t s);
// decode of B different conversations in one pass (RoPE + KV append fused): row t -> conversation row_slot[t] at position n_past[row_slot[t]], caches at
// kcache / vcache + row_slot[t] * seq_stride elements.
void launch_attn_llm_batched(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int B, int n_head, int hd, const int *n_past, const int *row_slot,
                             size_t seq_stride, int n_ctx, const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, hipStream_t s, int vs = 1);
// per row r, slot = row_slot[r]: argmax[slot] = feed[slot] = argmax(logits[r]); slot_logits[slot] = logits[r]; n_past[slot] += 1
void launch_batch_finish(const float *logits, int n_vocab, int B, const int *row_slot, int *n_past, int *argmax, int *feed, float *slot_logits, hipStream_t s);
void launch_batch_begin(int *n_past, const int *row_slot, const int *row_pos, int B, hipStream_t s);   // n_past[row_slot[r]] = row_pos[r]
// ---- verify pass: R <= DRAFT_ROWS rows of ONE conversation (row_slot[0]) at consecutive positions in one weight pass (Engine::verify_draft) ----
constexpr int DRAFT_ROWS = 8;                          // the conversation's greedy token + at most 7 draft tokens
// row t at position n_past[row_slot[0]] + t (all below n_ctx): RoPE + append of its own row, attention over the cache below the position, the pass's rows 0 .. t - 1
// and itself.  out and the appended rows are bit for bit those of R one-row launch_attn_llm_batched calls with n_past advanced by one between them.  n_past is not written.
// n_ctx <= attn_draft_max_ctx(hd) (below).
void launch_attn_llm_draft(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int R, int n_head, int hd, const int *n_past, const int *row_slot,
                           size_t seq_stride, int n_ctx, const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, hipStream_t s, int vs = 1);
void launch_draft_begin(int *n_past, const int *row_slot, const int *row_pos, hipStream_t s);   // n_past[row_slot[0]] = row_pos[0]
// res[1 + r] = first argmax of logits row r; m = leading draft tokens accepted (tok[i + 1] == res[1 + i], i < m); slot = row_slot[0]: slot_logits[slot] = logits[m],
// argmax[slot] = feed[slot] = res[1 + m], n_past[slot] += 1 + m, res[0] = m.  res: 1 + DRAFT_ROWS ints
void launch_draft_finish(const float *logits, int n_vocab, int R, const int *tok, const int *row_slot, int *n_past, int *argmax, int *feed, float *slot_logits, int *res, hipStream_t s);
// ---- verify pass of SEVERAL conversations (Engine::verify_draft_batch): N <= ATTN_MDRAFT_ROWS packed rows in consecutive groups, group g = R_g <= DRAFT_ROWS rows of
// conversation slot_g at positions p0_g + 0 .. R_g - 1, all slots distinct.  Nothing but row_slot [N] / row_pos [N] describes the grouping ----
constexpr int ATTN_MDRAFT_ROWS = 64;                   // the staging slab's rows
// n_past[slot_g] = p0_g (the position of each group's first row): ahead of the pass, where launch_draft_begin stands for one conversation
void launch_mdraft_begin(int *n_past, const int *row_slot, const int *row_pos, int N, hipStream_t s);
// row t (index r = row_pos[t] - n_past[row_slot[t]] in its group): RoPE + append of its own row, attention over its conversation's cache below p0, the group's rows
// before it and itself.  out and the appended rows are bit for bit those of one launch_attn_llm_draft per group; other conversations' caches and rows outside
// [p0_g, p0_g + R_g) are not written; a row at or past n_ctx stores nothing.  n_past is not written.  n_ctx <= attn_draft_max_ctx(hd).
void launch_attn_llm_draft_batched(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int N, int n_head, int hd, const int *n_past, const int *row_slot,
                                   const int *row_pos, size_t seq_stride, int n_ctx, const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, hipStream_t s, int vs = 1);
// res = m [ATTN_MDRAFT_ROWS] | row_greedy [ATTN_MDRAFT_ROWS].  row_greedy[t] = first argmax of logits row t; per group (first packed row t0, R rows, slot): m = leading
// draft tokens accepted (tok[t0 + i + 1] == row_greedy[t0 + i], i < m), slot_logits[slot] = logits[t0 + m], argmax[slot] = feed[slot] = row_greedy[t0 + m],
// n_past[slot] += 1 + m, m[t0] = m; m[t] = -1 for a row that is not a group's first.
void launch_draft_finish_batch(const float *logits, int n_vocab, int N, const int *tok, const int *row_slot, int *n_past, int *argmax, int *feed, float *slot_logits, int *res,
                               hipStream_t s);
// ---- prompt rows of several conversations packed in one chunk (Engine::prefill_batch) ----
// rows: device [N][2] = (slot, absolute position) per packed row.  k_rope_kv's arithmetic; cache row = position in kcache / vcache + slot * seq_stride
void launch_rope_kv_seg(float *q, const float *k, const float *v, int N, int n_head, int hd, const int *rows, size_t seq_stride, const float *cos_tab, const float *sin_tab,
                        __half *kcache, __half *vcache, hipStream_t s);
void launch_rope_kv_seg_slabs(const SlabSrc &src, int N, int n_head, int hd, const int *rows, size_t seq_stride, const float *cos_tab, const float *sin_tab, __half *kcache, __half *vcache,
                              hipStream_t s);   // n == 3, as launch_rope_kv_slabs
// segs: device [n_seg][4] = (slot, first packed row, rows, position of the first row); tiles[0] / [1]: device work lists of 16- / 32-query tiles built by attn_seg_tiles
// from the same (host) table; t_max >= every segment's position + rows (sizes the LDS score rows)
struct AttnSegs { const int *segs = nullptr; const int *tiles[2] = {nullptr, nullptr}; int n_tiles[2] = {0, 0}; int t_max = 0; size_t seq_stride = 0; };
int attn_seg_tiles(const int *segs, int n_seg, int qt, int *out);   // host: out[2 k] = segment, out[2 k + 1] = first query, longest first; returns the count
// one launch of the SEG form of k_attn_prefill_h8 / k_attn_prefill_h (same choice rule as launch_attn_prefill); each row bit-identical to its segment's own launch.
// false -> declined (the exact-f32 kernel is selected, or the score rows do not fit LDS): the caller runs per-segment launches.  out_h as launch_attn_prefill
bool launch_attn_prefill_seg(const float *q, const __half *kcache, const __half *vcache, const AttnSegs &sg, int n_head, int hd, const Tables &tb, float *out, const LaunchTuning &tune,
                             hipStream_t s, __half *out_h = nullptr, bool *wrote_h = nullptr);
// row r: logits row r belongs to conversation fin[2 r]: slot_logits / argmax / feed as launch_batch_finish, n_past[slot] = fin[2 r + 1]
void launch_seg_finish(const float *logits, int n_vocab, int B, const int *fin, int *n_past, int *argmax, int *feed, float *slot_logits, hipStream_t s);
void launch_gather_rows(const float *src, const int *idx, int n, int E, float *dst, hipStream_t s);   // dst[r] = src[idx[r]], rows of E floats
// scoring, one workgroup per row r of `logits` (row stride ld >= n_vocab floats, any alignment): greedy[r] = first argmax, greedy_logprob[r] = its log-softmax,
// logprob[r] = log softmax(row)[targets[r]] (natural logarithm; the maximum is subtracted before exp), or 0 when targets[r] == -1
void launch_logprob_rows(const float *logits, int ld, int n_vocab, int rows, const int *targets, float *logprob, int *greedy, float *greedy_logprob, hipStream_t s);
// top-N alternatives, one workgroup per row r of `logits` (read at logits + (row_index ? row_index[r] : r) * ld; any 4-byte alignment, duplicates allowed):
// ids[r][0, top_n) = the first top_n tokens in the order "logit descending, equal logits (float equality: -0 and +0 tie) by ascending id", logprobs[r][j] = the
// log-softmax of ids[r][j] -- bit for bit what launch_logprob_rows reports for that token as the row's target --, rank[r] = how many tokens sort before targets[r]
// (-1 without a target), target_logprob[r] = launch_logprob_rows' logprob (0 without a target).  Outputs are packed [rows][top_n].  The number of sweeps over a row
// does not depend on top_n or on the data (llm_kernels.hip).  false + last_error: rows / n_vocab < 1, ld < n_vocab, top_n outside [1, min(TOPN_MAX, n_vocab)]
constexpr int TOPN_MAX = 64;   // one wavefront of candidates above the threshold; covers the reference's default top-k of 40
bool launch_topn_rows(const float *logits, int ld, int n_vocab, int rows, const int *row_index, int top_n, const int *targets, int *ids, float *logprobs, int *rank,
                      float *target_logprob, hipStream_t s);
// one beam-search step's decision (beam.hpp: the rule), one workgroup: ids / logprobs = [W][C] as launch_topn_rows just wrote them (top_n = C), scores[W] the beams'
// cumulative scores, live bit i = beam i takes part.  Writes *res (the step's parents, tokens, scores and the hypotheses EOS finished), scores[i] = res->score[i] for the
// next step and row_tok[i] = res->tok[i] -- where the batched step reads its row tokens (an id outside [0, n_vocab) is written as 0: it indexes the embedding matrix).
// false + last_error: W outside 2 .. BEAM_MAX, C outside 1 .. BEAM_CAND_MAX, no live beam
bool launch_beam_select(const int *ids, const float *logprobs, float *scores, unsigned live, int W, int C, int eos, int n_vocab, BeamStep *res, int *row_tok, hipStream_t s);
// ---- the device picks: launch_pen_pick, launch_constrain_pick, launch_sample_rows.  One workgroup per entry of `rows` (device).  THE TRANSFORMED ROW of an entry, walked
// by all three the same way (pick_row.hpp): logits row pen.row (at logits + row * ld, any 4-byte alignment) after the bias / repetition / frequency / presence
// transformation its table entries table[pen.off .. + pen.n) describe (penalty.hpp; distinct ids, one outside [0, n_vocab) is ignored; pen.n == 0: none), restricted to the
// ids set in the entry's `allowed` bitmap where it has one (constraint_words(n_vocab) words, device; null: every id).  The logits are not written.
// penalised greedy pick: picked[r] = the first maximum of the transformed row (0 for a row without a comparable value).  adjusted (may be null): [table entry] the transformed value.  false + last_error: n_rows / n_vocab < 1, ld < n_vocab, a vocabulary whose
// bitmap does not fit LDS
bool launch_pen_pick(const float *logits, int ld, int n_vocab, int n_rows, const PenRow *rows, const PenEntry *table, int *picked, float *adjusted, hipStream_t s);
// constrained decoding (constraint.hpp).  launch_constrain_index: index[n_states][constraint_words(n_vocab)] = the allowed-token bitmap of every DFA state, one workgroup per
// state; vocab / off[n_vocab + 1] = the pieces' bytes back to back and where each begins (device), trans[n_states][256] with entries < n_states, accept = the accepting
// bitmap.  false + last_error: a null array, n_vocab < 1, n_states outside 2 .. CONSTRAINT_MAX_STATES.
// launch_constrain_pick: out[r] = the first maximum of the transformed row (above) under rows[r].allowed; no id set: CONSTRAINT_EOS | CONSTRAIN_STUCK.
// false + last_error: a null array, n_rows / n_vocab < 1, ld < n_vocab, a vocabulary whose two bitmaps do not fit LDS.
constexpr int CONSTRAIN_STUCK = 1 << 30;               // flag in a pick's output word: the row had no allowed id
struct ConRow { PenRow pen; const unsigned *allowed; unsigned long long pad; };   // 12 words
bool launch_constrain_index(const unsigned char *vocab, const int *off, int n_vocab, const uint16_t *trans, const unsigned *accept, int n_states, unsigned *index, hipStream_t s);
bool launch_constrain_pick(const float *logits, int ld, int n_vocab, int n_rows, const ConRow *rows, const PenEntry *table, int *out, hipStream_t s);
// guided decoding, one workgroup per entry of `pairs` (device), n_pairs <= GUIDE_MAX: b = logits row pos_row, g = row neg_row (at logits + row * ld, any 4-byte alignment;
// the two may be one row, a row may serve several pairs), m[j] = lg[j] + scale * (lb[j] - lg[j]) with lb / lg the rows' log-softmax -- bit for bit launch_topn_rows'
// log-probabilities -- and every operation rounded to fp32 on its own.  mixed (may be null): [n_pairs][n_vocab] = m; pick[p] = the first maximum of m, pick_val[p] = m[pick];
// row_tok (may be null): row_tok[pos_tok] = row_tok[neg_tok] = pick for the indices that are >= 0 (the row tokens of the batched step that follows in the stream).  The
// logits are not written.  false + last_error: n_pairs outside 1 .. GUIDE_MAX, n_vocab < 1, ld < n_vocab, a null table / pick / pick_val
constexpr int GUIDE_MAX = 32;                          // pairs per launch = Engine::MAX_CONVERSATIONS / 2
struct GuidePair { int pos_row, neg_row; float scale; int pos_tok, neg_tok, pad[3]; };   // 8 words
bool launch_guide_rows(const float *logits, int ld, int n_vocab, int n_pairs, const GuidePair *pairs, float *mixed, int *pick, float *pick_val, int *row_tok, hipStream_t s);
// sampled decode step (sampling.hpp: the generator and the rule): the first min(top_k, participating ids) ids of the transformed row (above) under rows[r].allowed, in
// launch_topn_rows' order; top-p, temperature and softmax over them; one draw with word 0 of Philox4x32-10(seed, draws).  out[r] = pick, stuck flag, word,
// n_cand, kept, ids, probabilities; row_tok (may be null): row_tok[rows[r].tok_index] = pick where the index is >= 0.  top_k is clamped to
// 1 .. SAMPLE_MAX; temp > 0 and 0 < top_p are the caller's to check.  false + last_error: a null array, n_rows / n_vocab < 1, ld < n_vocab, a vocabulary whose two bitmaps
// and the kernel's 12 KB do not fit 64 KB of LDS.
struct SampleRow { PenRow pen; const unsigned *allowed; float temp, top_p; int top_k, tok_index; unsigned long long seed, draws; };   // 18 words
bool launch_sample_rows(const float *logits, int ld, int n_vocab, int n_rows, const SampleRow *rows, const PenEntry *table, SampleOut *out, int *row_tok, hipStream_t s);
// the same decision under the extended rule (sampling.hpp: sample_chain): the selection is launch_sample_rows', then tail-free, typical, top-p, min-p, temperature,
// softmax and the draw over the live list -- or mirostat v2 over the candidates, from rows[r].chain.mu (NaN: 2 * tau).  out[r] = the plain result (kept = the
// live list's length), then the 64-bit mask of the candidates left in it, mu' (mirostat 0: mu as given) and the observed surprise.  The chain's ranges (tfs_z and
// typical_p in (0, 1], min_p in [0, 1], mirostat 0 or 2, tau > 0, eta >= 0) are the caller's to check.  Refusals as launch_sample_rows.
struct SampleRowEx { SampleRow base; ChainParams chain; };   // 26 words
bool launch_sample_rows_ex(const float *logits, int ld, int n_vocab, int n_rows, const SampleRowEx *rows, const PenEntry *table, SampleOutEx *out, int *row_tok, hipStream_t s);
// verify pass epilogue under sampling, behind launch_sample_rows over the pass's R rows (picks[r] = the decision of logits row r, rows ld floats apart; tok[0 .. R) = the
// pass's row tokens): m = the leading draft tokens the rows' own samples chose (tok[i + 1] == picks[i].pick); the logits of row m -> slot_logits[slot], slot = row_slot[0],
// argmax[slot] = feed[slot] = the first maximum of that row, n_past[slot] += 1 + m; res = {m, picks [DRAFT_ROWS], stuck flags [DRAFT_ROWS]}, 1 + 2 DRAFT_ROWS ints.
// false + last_error: a null array, R outside 1 .. DRAFT_ROWS, n_vocab < 1, ld < n_vocab.
constexpr int DRAFT_SAMPLE_RES = 1 + 2 * DRAFT_ROWS;
bool launch_draft_sample_finish(const float *logits, int ld, int n_vocab, int R, const int *tok, const SampleOut *picks, const int *row_slot, int *n_past, int *argmax, int *feed,
                                float *slot_logits, int *res, hipStream_t s);
// the same behind launch_sample_rows_ex (picks: its extended blocks)
bool launch_draft_sample_finish(const float *logits, int ld, int n_vocab, int R, const int *tok, const SampleOutEx *picks, const int *row_slot, int *n_past, int *argmax, int *feed,
                                float *slot_logits, int *res, hipStream_t s);
// prefill (N > 1 rows of one conversation, after launch_rope_kv): workgroup = (head, 16 queries), keys streamed through LDS in tiles, exact-f32 MFMA; t_max >= *n_past + N
// sizes the LDS score rows; false -> does not fit (the caller uses launch_attn_llm)
// out_h (optional): a kernel that can do so stores the fp16-rounded rows THERE instead of fp32 rows in `out` and sets *wrote_h (the F16 wo's input rows)
bool launch_attn_prefill(const float *q, const __half *kcache, const __half *vcache, int N, int n_head, int hd, const int *n_past, int t_max, const Tables &tb, float *out, const LaunchTuning &tune, hipStream_t s, __half *out_h = nullptr, bool *wrote_h = nullptr);
// MINIGPT4_PARITY=1: scores / softmax / P.V with every fp32 chain in the oracle's order (after launch_rope_kv); t_max >= *n_past + N
void launch_attn_ref(const float *q, const __half *kcache, const __half *vcache, int N, int n_head, int hd, const int *n_past, int t_max, const Tables &tb, float *out, hipStream_t s);
void launch_attn_ref_fused(const float *q, const float *k, const float *v, __half *kcache, __half *vcache, int n_head, int hd, const int *n_past, int t_max, const float *cos_tab, const float *sin_tab,
                           const Tables &tb, float *out, hipStream_t s);   // one query row: RoPE + cache append inside
bool attn_head_size_supported(int hd);
void attn_ref_prepare();        // the oracle-order attention kernels' > 64 KiB LDS opt-in on the current device, checked (throws HipError); outside any stream capture
int attn_ref_max_ctx(int hd);   // the same bound for the oracle-order kernel of parity mode (smaller: it also stages value rows in LDS)
int attn_max_ctx(int hd);   // largest n_ctx whose score / probability rows fit the attention kernel's LDS
int attn_draft_max_ctx(int hd);   // the same bound for the verify form (launch_attn_llm_draft), which keeps DRAFT_ROWS new key / value rows in LDS instead of one: smaller
void launch_argmax(const float *logits, int n, int *out, void *scratch /*>= 512 bytes*/, hipStream_t s);
void launch_add_inplace(float *x, const float *y, size_t n, hipStream_t s);
void launch_set_int(int *p, int v, hipStream_t s);
void launch_stall(unsigned ms, hipStream_t s);   // test injection: a bounded (<= 5 s) busy kernel
uint64_t device_checksum(const void *p, size_t bytes, hipStream_t s);   // sum of the 32-bit words (bytes rounded down to 4), mod 2^64; synchronises the stream
void launch_fill_u16(void *p, size_t n, unsigned short v, hipStream_t s);
void launch_advance(int *n_past, int n, int *tok0, const int *argmax, hipStream_t s);
void launch_delay(int us, hipStream_t s);   // profiling gate: keeps the stream busy for `us` microseconds (see Engine::profile_sites)

// ---- vision tower -----------------------------------------------------------------------------------------------------
// C[M][N] = A[M][K](f16) . W[N][K](f16)^T + bias ; optional fp16-table GELU ; optional residual add (C = residual + C).
// Writes fp32 `out` (nullable) and/or fp16 `out_h` (nullable).  K must be a multiple of 16.
void launch_gemm_f16(const __half *A, int lda, const __half *W, int ldw, int M, int N, int K, const float *bias, const float *residual,
                     bool gelu, const Tables &tb, float *out, __half *out_h, int ldo, const LaunchTuning &tune, hipStream_t s);
// fp32 output stored [N / D][D / hd][M][hd] (the ViT's qkv projection for k_attn_vit's head strides; vision_kernels.hip: struct HeadMajor)
void launch_gemm_f16_head_major(const __half *A, int lda, const __half *W, int ldw, int M, int N, int K, const float *bias, const Tables &tb, float *out, int D, int hd, const LaunchTuning &tune, hipStream_t s);
// out = [residual +] gelu?(bias + y) over [rows][n] contiguous fp32 (y may alias out); writes fp32 (nullable) and / or fp16 (nullable)
// the same product for FEW rows (the Q-Former's 32 queries per image): N / 16 workgroups, K split across the waves of a workgroup, no LDS staging.  false -> shape outside
// the kernel's range (N % 16, K % 32), nothing launched
bool launch_gemm_f16_skinny(const __half *A, int lda, const __half *W, int ldw, int M, int N, int K, const float *bias, const float *residual, bool gelu, const Tables &tb,
                            float *out, __half *out_h, int ldo, hipStream_t s);
bool launch_gemm_f16_skinny_splitk(const __half *A, int lda, const __half *W, int ldw, int M, int N, int K, int slices, float *slabs, size_t slab_stride, int ldo, hipStream_t s);   // raw partial sums per K slice -> launch_splitk_reduce_ln
void launch_lin_epilogue(const float *y, const float *bias, const float *residual, bool gelu, const Tables &tb, int rows, int n, float *out, __half *out_h, hipStream_t s);
// LayerNorm (ggml_norm eps 1e-5, then w*x+b); rows x n; writes fp32 (nullable) and fp16 (nullable).
void launch_layernorm(const float *x, const float *w, const float *b, int rows, int n, float *out, __half *out_h, hipStream_t s, bool sequential_sums = false);   // sequential_sums: MINIGPT4_PARITY
// MINIGPT4_PARITY: ViT / BERT attention with every fp32 chain in the oracle's order (fp32 output); same argument meaning as launch_attn_f32
void launch_attn_vref(const float *q, int ldq, const float *k, const float *v, int ldk, int nq, int nk, int heads, int hd, float q_prescale, float score_div, const Tables &tb,
                      float *out, int ldo, hipStream_t s, int batch = 1);
// split-K GEMM (raw fp32 partial sums into `slices` slabs) + the deterministic reduce fused with bias / residual / the following LayerNorm
bool launch_gemm_f16_arm(int arm, const __half *A, int lda, const __half *W, int ldw, int M, int N, int K, const float *bias, const float *residual, bool gelu, const Tables &tb,
                         float *out, __half *out_h, int ldo, const LaunchTuning &tune, hipStream_t s);   // micro-benchmark arms (other tile shapes of k_gemm_f16)
bool launch_gemm_f16_splitk_arm(int arm, const __half *A, int lda, const __half *W, int ldw, int M, int N, int K, int slices, float *slabs, size_t slab_stride, int ldo, const LaunchTuning &tune, hipStream_t s);
int gemm_split_slices(int K, int want);   // slices actually used for a K (whole 128-wide k tiles per slice)
void launch_gemm_f16_splitk(const __half *A, int lda, const __half *W, int ldw, int M, int N, int K, int slices, float *slabs, size_t slab_stride, int ldo, const LaunchTuning &tune, hipStream_t s);
void launch_splitk_reduce_ln(const float *slabs, int n_slabs, size_t slab_stride, const float *bias, const float *residual, int rows, int n, float *x_out, const float *ln_w,
                             const float *ln_b, float *ln_out, __half *ln_out_h, hipStream_t s);
// f32 attention: q[nq][ldq], k/v[nk][ldk]; per head h the slice [h*hd, (h+1)*hd).  q_prescale != 0: q *= q_prescale first (ViT);
// score_div != 0: scores /= score_div (BERT).  Output fp32 (nullable) / fp16 (nullable) [nq][ldo].
// batch > 1: image z uses rows [z * nq, (z + 1) * nq) of q / out and rows [z * nk, (z + 1) * nk) of k / v.
void launch_attn_f32(const float *q, int ldq, const float *k, const float *v, int ldk, int nq, int nk, int heads, int hd, float q_prescale,
                     float score_div, const Tables &tb, float *out, __half *out_h, int ldo, const LaunchTuning &tune, hipStream_t s, int batch = 1, int head_stride_q = 0, int head_stride_kv = 0)   /* head strides in floats; 0 = hd (heads side by side in a row) */;
// image CHW f32 [3][224][224] -> fp16 patches [256][ldp] (k = c*196 + kh*14 + kw, zero padded to ldp)
void launch_im2col(const float *image, __half *patches, int ldp, hipStream_t s, int batch = 1);   // batch images back to back -> [batch * 256][ldp]
// x[0] = cls + pos[0]; x[1+p] = pe[p] + pos[1+p]
void launch_assemble_embeddings(const float *cls, const float *pe, const float *pos, int D, float *x, hipStream_t s, int batch = 1);
void launch_f32_to_f16(const float *x, __half *y, size_t n, hipStream_t s);

// ---- image preprocess (image_kernels.hip): Pillow's 8-bit bicubic resample, horizontal then vertical pass, all pointers device ---------------
// dst[y][xx][c] = clip8(2^21 + sum_i src[y][first[xx] + i][c] * kk[xx * ksize + i] >> 22); src [H][W][3], dst [H][OW][3]
void launch_resample_h(const uint8_t *src, int W, int H, const int *first, const int *count, const int *kk, int ksize, uint8_t *dst, int OW, hipStream_t s);
// vertical pass over src [*][OW][3] fused with x * (1/255), (x - mean) / std and HWC -> CHW: out [3][OH][OW] f32
void launch_resample_v_norm(const uint8_t *src, int OW, const int *first, const int *count, const int *kk, int ksize, float *out, int OH, const float mean[3], const float std[3],
                            hipStream_t s);

}  // namespace mg4
