// extern "C" hooks of libminigpt4_test.so ONLY (include/minigpt4_amd_test.h): single-kernel parity hooks, micro-benchmarks, hardware probes and host-only helpers for
// the CPU test tier.  The product library (libminigpt4.so) is linked without this file: none of these symbols ship.
#include <sys/stat.h>

#include <chrono>
#include <cstring>

#include "api_internal.hpp"
#include "activations.hpp"
#include "draft.hpp"
#include "draft_host.hpp"
#include "beam_host.hpp"
#include "imageio.hpp"
#include "quantize.hpp"
#include "minigpt4_amd.h"
#include "minigpt4_amd_test.h"

using namespace mg4;
using namespace mg4::apiutil;

namespace mg4 {   // probe_kernels.hip
float probe_valu_ns(int op, int waves_per_simd, int iters, int cus);
float probe_grid_barrier_us(int n_blocks, int iters, unsigned *errors_out);
int parse_dist_env_for_test(int *world, int *rank, char *id_file, size_t cap, char *err, size_t err_cap);
float probe_dma_GBps(int form, int policy, int waves, int fill, int depth, int deal, size_t total_bytes);
void launch_fill_random(void *p, size_t bytes, unsigned seed, hipStream_t s);
}

// The launch tuning of the single-kernel hooks.  It lives in this library only and no context ever reads it (a context has its own: Engine::tune_).  The sticky setters
// Python calls (minigpt4_amd_test_set_gemm_arm / _set_splitk_xcd / _set_attn_qt) write it; a hook that varies a knob for ONE call works on hook_tuning()'s copy.
static LaunchTuning g_tune;
static LaunchTuning hook_tuning() { LaunchTuning t = g_tune; hipDeviceProp_t prop; HIP_CHECK(hipGetDeviceProperties(&prop, 0)); t.cus = prop.multiProcessorCount; return t; }

// One thread per fp16 bit pattern: the table functions of activations.hpp exactly as the kernels' epilogues call them (t == null: the computed form), result as fp16 bits.
// which: 0 GELU, 1 SiLU, 2 exp (the oracle's orc_table numbering)
__global__ __launch_bounds__(256) void k_test_activation(int which, const __half *t, unsigned short *out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= 65536u) return;
    const float x = h2f_bits((unsigned short)i);
    const float y = which == 0 ? gelu_h(t, x) : which == 1 ? silu_h(t, x) : exp_h(t, x);
    out[i] = f2h_bits(y);
}

// ggml's fp16 tables as the host libm gives them (the hooks' original entry points gather from these; the _ex forms take the caller's table or none)
static std::vector<unsigned short> host_gelu_table() {
    std::vector<unsigned short> g(65536);
    for (int i = 0; i < 65536; i++) { const float x = __half2float(__ushort_as_half((unsigned short)i)); g[(size_t)i] = __half_as_ushort(__float2half_rn(0.5f * x * (1.0f + tanhf(0.79788456080286535587989211986876f * x * (1.0f + 0.044715f * x * x))))); }
    return g;
}
static std::vector<unsigned short> host_silu_table() {
    std::vector<unsigned short> si(65536);
    for (int i = 0; i < 65536; i++) { const float v = __half2float(__ushort_as_half((unsigned short)i)); si[(size_t)i] = __half_as_ushort(__float2half_rn(v / (1.0f + expf(-v)))); }
    return si;
}
// the timed hooks' event pair (hipEventCreate on a and b; timing enabled), destroyed on every path
struct Events { hipEvent_t a = nullptr, b = nullptr; ~Events() { if (a) HIP_IGNORE(hipEventDestroy(a)); if (b) HIP_IGNORE(hipEventDestroy(b)); } };
// ONE timed region of the null stream: f() between two event records, the device awaited, the elapsed milliseconds -> *ms_out (may be null).  false: f() returned
// false (a launcher that refused): nothing was awaited
template <typename F> static bool timed(float *ms_out, F f) {
    Events ev;
    HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b));
    HIP_CHECK(hipEventRecord(ev.a, nullptr));
    if (!f()) return false;
    HIP_CHECK(hipEventRecord(ev.b, nullptr));
    HIP_CHECK(hipDeviceSynchronize());
    float t = 0; HIP_CHECK(hipEventElapsedTime(&t, ev.a, ev.b));
    if (ms_out) *ms_out = t;
    return true;
}
// Everything of a pick hook's descriptors that indexes device memory: rows = [n_rows] PenRow as 8 words, table = [n_table] PenEntry as 4 words.  Row index inside the
// buffer, offset and count inside the table, at most PEN_TABLE_MAX entries, every id inside the vocabulary, the ids of one row distinct
static bool pen_rows_ok(const int32_t *rows, int n_rows, const int32_t *table, int n_table, int buf_rows, int n_vocab) {
    for (int r = 0; r < n_rows; r++) {
        const int32_t *w = rows + 8 * (size_t)r;
        if (w[0] < 0 || w[0] >= buf_rows || w[1] < 0 || w[2] < 0 || w[2] > PEN_TABLE_MAX || (long long)w[1] + w[2] > n_table) return false;
        std::vector<int> ids;
        for (int i = 0; i < w[2]; i++) { const int id = table[4 * ((size_t)w[1] + i)]; if (id < 0 || id >= n_vocab) return false; ids.push_back(id); }
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return false;
    }
    return true;
}

extern "C" {

int minigpt4_amd_copy_arenas(struct MiniGPT4Context *dst, struct MiniGPT4Context *src) {   // single-GPU stand-in for the broadcast (tests): both weight arenas, device to device
    if (!dst || !src) return 1;
    return guarded(3, [&]() -> int {
        Engine *d = E_(dst), *s = E_(src);
        if (d->llm_arena_bytes() != s->llm_arena_bytes() || d->vision_arena_bytes() != s->vision_arena_bytes()) { set_last_error("arena sizes differ"); return 2; }
        HIP_CHECK(hipMemcpy(d->llm_arena_ptr(), s->llm_arena_ptr(), s->llm_arena_bytes(), hipMemcpyDeviceToDevice));
        HIP_CHECK(hipMemcpy(d->vision_arena_ptr(), s->vision_arena_ptr(), s->vision_arena_bytes(), hipMemcpyDeviceToDevice));
        return 0;
    });
}

// ---- single-kernel hooks ---------------------------------------------------------------------------------------------------

int minigpt4_amd_timeline_rows(unsigned long long *out, int max_workgroups) { return (out && max_workgroups > 0) ? read_matvec_timeline_rows(out, max_workgroups) : -1; }
int minigpt4_amd_timeline(unsigned long long *out, int max_workgroups) { return (out && max_workgroups > 0) ? read_matvec_timeline(out, max_workgroups) : -1; }

int minigpt4_amd_convert_q3k_q6k(const void *src, void *dst, int64_t n_blocks) {
    if (!src || !dst || n_blocks < 0) return 1;
    q3k_to_q6k(static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), (size_t)n_blocks);
    return 0;
}

static int test_mul_mat_impl(int ggml_type, const void *raw_w, int64_t n_in, int64_t n_out, const float *x, int64_t N, float *y, bool ref);
int minigpt4_amd_test_mul_mat(int ggml_type, const void *raw_w, int64_t n_in, int64_t n_out, const float *x, int64_t N, float *y) { return test_mul_mat_impl(ggml_type, raw_w, n_in, n_out, x, N, y, false); }
int minigpt4_amd_test_mul_mat_ref(int ggml_type, const void *raw_w, int64_t n_in, int64_t n_out, const float *x, int64_t N, float *y) { return test_mul_mat_impl(ggml_type, raw_w, n_in, n_out, x, N, y, true); }
static int test_mul_mat_impl(int ggml_type, const void *raw_w, int64_t n_in, int64_t n_out, const float *x, int64_t N, float *y, bool ref) {
    if (ggml_type == GT_Q3_K && raw_w && n_in > 0 && n_out > 0 && n_in % 256 == 0) {   // the engine's load path: exact Q6_K image (quantize.hpp)
        std::vector<uint8_t> q6((size_t)(n_in / 256 * n_out) * 210);
        q3k_to_q6k(static_cast<const uint8_t *>(raw_w), q6.data(), (size_t)(n_in / 256 * n_out));
        return test_mul_mat_impl(GT_Q6_K, q6.data(), n_in, n_out, x, N, y, ref);
    }
    if (!raw_w || !x || !y || n_in <= 0 || n_out <= 0 || N <= 0 || !qweight_supported(ggml_type) || n_in % gt_block(ggml_type)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t raw_bytes = gt_nbytes(ggml_type, (size_t)(n_in * n_out));
        QWeight W, plan;
        const size_t need = plan_qweight(ggml_type, (int)n_out, (int)n_in, plan, nullptr);
        DevBuf d_raw(raw_bytes), d_planes(need), d_x((size_t)(N * n_in) * 4), d_y((size_t)(N * n_out) * 4);
        plan_qweight(ggml_type, (int)n_out, (int)n_in, W, d_planes.as<uint8_t>());
        HIP_CHECK(hipMemcpy(d_raw.p, raw_w, raw_bytes, hipMemcpyHostToDevice));
        if (ggml_type == GT_F16 || ggml_type == GT_F32) HIP_CHECK(hipMemcpy(d_planes.p, raw_w, raw_bytes, hipMemcpyHostToDevice)); else launch_repack(d_raw.as<uint8_t>(), W, nullptr);
        HIP_CHECK(hipMemcpy(d_x.p, x, (size_t)(N * n_in) * 4, hipMemcpyHostToDevice));
        ActQ A; std::vector<std::unique_ptr<DevBuf>> keep; alloc_act(A, keep, (size_t)N, (size_t)n_in);
        launch_rms_quant(d_x.as<float>(), nullptr, (int)N, (int)n_in, A, act_mask_for(ggml_type), nullptr);
        if (ref) launch_mul_mat_ref(W, A, (int)N, d_y.as<float>(), (int)n_out, nullptr, g_tune, nullptr);
        else launch_mul_mat(W, A, (int)N, d_y.as<float>(), (int)n_out, nullptr, g_tune, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(y, d_y.p, (size_t)(N * n_out) * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// The prefill launch of Engine::forward for N > 4 rows (mmq2_kernels.hip): n_mat equally shaped matrices (rows of `raw_w` back to back) against N rows in ONE launch, optional
// residual ([n_mat][N][n_out]), optional forced K split (ks > 1: partial sums combined in fixed order).  y: [n_mat][N][n_out].  Returns 4 when the kernels refuse the shape.
int minigpt4_amd_test_mmq2(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int64_t N, const float *residual, int ks, int generation, float *y) {
    if (!raw_w || !x || !y || n_in <= 0 || n_out <= 0 || N <= 0 || n_mat < 1 || n_mat > 3 || !qweight_supported(ggml_type) || n_in % gt_block(ggml_type)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t raw_each = gt_nbytes(ggml_type, (size_t)(n_in * n_out)), out_each = (size_t)(N * n_out);
        QWeight W[3], plan;
        const size_t need = plan_qweight(ggml_type, (int)n_out, (int)n_in, plan, nullptr);
        DevBuf d_raw(raw_each), d_planes(need * (size_t)n_mat + 1024), d_x((size_t)(N * n_in) * 4), d_y(out_each * n_mat * 4), d_res(out_each * n_mat * 4), d_ws(out_each * n_mat * 16 * 4);
        for (int i = 0; i < n_mat; i++) {
            plan_qweight(ggml_type, (int)n_out, (int)n_in, W[i], d_planes.as<uint8_t>() + (size_t)i * need);
            HIP_CHECK(hipMemcpy(d_raw.p, static_cast<const uint8_t *>(raw_w) + (size_t)i * raw_each, raw_each, hipMemcpyHostToDevice));
            launch_repack(d_raw.as<uint8_t>(), W[i], nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        }
        HIP_CHECK(hipMemcpy(d_x.p, x, (size_t)(N * n_in) * 4, hipMemcpyHostToDevice));
        if (residual) HIP_CHECK(hipMemcpy(d_res.p, residual, out_each * n_mat * 4, hipMemcpyHostToDevice));
        ActQ A; std::vector<std::unique_ptr<DevBuf>> keep; alloc_act(A, keep, (size_t)N, (size_t)n_in);
        launch_rms_quant(d_x.as<float>(), nullptr, (int)N, (int)n_in, A, act_mask_for(ggml_type), nullptr);
        const QWeight *Wp[3]; float *Yp[3]; const float *Rp[3];
        for (int i = 0; i < n_mat; i++) { Wp[i] = &W[i]; Yp[i] = d_y.as<float>() + (size_t)i * out_each; Rp[i] = d_res.as<float>() + (size_t)i * out_each; }
        A.ws = d_ws.as<float>(); A.ws_floats = out_each * n_mat * 16;
        bool ok;
        LaunchTuning tune = hook_tuning();
        tune.f16_ks = tune.mmq_ks = ks; tune.mmqh = generation == 4;   // 4: k_mmqh_q45k (fp16-MFMA form, not adopted)
        tune = tune.normalised();
        if (ggml_type == GT_F16) {   // the F16 language-model set path (big MFMA GEMM, several matrices per launch / split K)
            const __half *Wh[3]; for (int i = 0; i < n_mat; i++) Wh[i] = reinterpret_cast<const __half *>(W[i].qs);
            ok = launch_gemm_f16_set(A.xh, (int)n_in, Wh, n_mat, (int)N, (int)n_out, (int)n_in, Yp, residual ? Rp : nullptr, (int)n_out, A.ws, A.ws_floats, tune, nullptr);
        } else {
            if (generation == 3) {   // load-time digit planes (mmq3_kernels.hip)
                if (!mmq3_supported(ggml_type, (int)n_out, (int)n_in)) return 4;
                const size_t pb = mmq3_plane_bytes((int)n_out, (int)n_in);
                DevBuf d_pl(pb * (size_t)n_mat);
                const uint8_t *Pp[3];
                for (int i = 0; i < n_mat; i++) { Pp[i] = d_pl.as<uint8_t>() + (size_t)i * pb; launch_mmq3_build(W[i], d_pl.as<uint8_t>() + (size_t)i * pb, nullptr); }
                ok = launch_mmq3_set(Wp, Pp, Yp, residual ? Rp : nullptr, n_mat, A, (int)N, (int)n_out, tune, nullptr);
                HIP_CHECK(hipDeviceSynchronize());
            } else ok = launch_mmq2_set(Wp, Yp, residual ? Rp : nullptr, n_mat, A, (int)N, (int)n_out, tune, nullptr);
        }
        HIP_CHECK(hipDeviceSynchronize());
        if (!ok) return 4;
        HIP_CHECK(hipMemcpy(y, d_y.p, out_each * n_mat * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// The decode mat-vec launches exactly as Engine::forward issues them: n1 equally spaced matrices of type1 (+ optionally n2 of type2 in the same,
// mixed-type launch), activation preparation either standalone (fuse = 0) or in the kernel prologue, optional residual, optional SiLU row-pair
// epilogue.  prep: 1 = rms_norm(x) * x2, 2 = x, 3 = silu(x) * x2.  y: (n1 + n2) * n_out floats (epi = 1: n_out floats).
static int test_matvec_impl(int type1, const void *raw1, int n1, int type2, const void *raw2, int n2, int64_t n_in, int64_t n_out, const float *x, const float *x2, int prep,
                            int fuse, int epi, const float *residual, const unsigned short *silu_table, float *y, bool issue_bar = false, int guard = 0);
int minigpt4_amd_test_matvec(int type1, const void *raw1, int n1, int type2, const void *raw2, int n2, int64_t n_in, int64_t n_out, const float *x, const float *x2, int prep,
                             int fuse, int epi, const float *residual, float *y) {
    return test_matvec_impl(type1, raw1, n1, type2, raw2, n2, n_in, n_out, x, x2, prep, fuse, epi, residual, host_silu_table().data(), y);
}
// silu_table: the table of prep = 3 / epi = 1, or NULL: Tables::silu stays null -- the computed arm, as Engine::tabs_dec_ passes it to the decode step's launches
int minigpt4_amd_test_matvec_ex(int type1, const void *raw1, int n1, int type2, const void *raw2, int n2, int64_t n_in, int64_t n_out, const float *x, const float *x2, int prep,
                                int fuse, int epi, const float *residual, const unsigned short *silu_table, float *y) {
    // the mat-vec's fused SiLU prologue and its pair epilogue always gather (the engine hands them the tables): only the stand-alone preparation launch has a computed arm
    if (!silu_table && ((fuse && prep == 3) || epi == 1)) { set_last_error("the fused SiLU prologue / pair epilogue of the decode mat-vec need a table"); return 1; }
    return test_matvec_impl(type1, raw1, n1, type2, raw2, n2, n_in, n_out, x, x2, prep, fuse, epi, residual, silu_table, y);
}
// ONE prologue launch (the preparation fused, as the decode step issues it) with or without the issue barrier.  y: the outputs followed by `guard` floats behind them,
// which the launch must leave at the 0xFF bytes they were filled with.
int minigpt4_amd_test_matvec_issue(int type1, const void *raw1, int n1, int type2, const void *raw2, int n2, int64_t n_in, int64_t n_out, const float *x, const float *x2, int prep,
                                   int epi, const float *residual, int issue_barrier, int guard, float *y) {
    if (guard < 0 || guard > (1 << 20)) return 1;
    return test_matvec_impl(type1, raw1, n1, type2, raw2, n2, n_in, n_out, x, x2, prep, 1, epi, residual, host_silu_table().data(), y, issue_barrier != 0, guard);
}
int minigpt4_amd_test_matvec_waves(void) { return matvec_prologue_waves(g_tune); }
static int test_matvec_impl(int type1, const void *raw1, int n1, int type2, const void *raw2, int n2, int64_t n_in, int64_t n_out, const float *x, const float *x2, int prep,
                            int fuse, int epi, const float *residual, const unsigned short *silu_table, float *y, bool issue_bar, int guard) {
    if (!raw1 || !x || !y || n_in <= 0 || n_out <= 0 || n1 < 1 || n1 > 3 || n2 < 0 || n2 > 1 || prep < 1 || prep > 3 || (prep != 2 && !x2)) return 1;
    if (!qweight_supported(type1) || n_in % gt_block(type1) || (n2 && (!raw2 || !qweight_supported(type2) || n_in % gt_block(type2)))) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int K = (int)n_in, R = (int)n_out, nt = n1 + n2;
        std::vector<std::unique_ptr<DevBuf>> keep;
        std::vector<QWeight> W((size_t)nt);
        auto upload = [&](int type, const void *raw, int n, QWeight *dst) {
            QWeight plan; const size_t need = plan_qweight(type, R, K, plan, nullptr), raw_bytes = gt_nbytes(type, (size_t)R * K);
            keep.emplace_back(new DevBuf(need * (size_t)n)); uint8_t *base = (uint8_t *)keep.back()->p;   // one allocation: equal spacing
            DevBuf d_raw(raw_bytes);
            for (int m = 0; m < n; m++) {
                plan_qweight(type, R, K, dst[m], base + (size_t)m * need);
                HIP_CHECK(hipMemcpy(d_raw.p, (const uint8_t *)raw + (size_t)m * raw_bytes, raw_bytes, hipMemcpyHostToDevice));
                if (type == GT_F16 || type == GT_F32) HIP_CHECK(hipMemcpy(base + (size_t)m * need, d_raw.p, raw_bytes, hipMemcpyDeviceToDevice)); else launch_repack(d_raw.as<uint8_t>(), dst[m], nullptr);
                HIP_CHECK(hipDeviceSynchronize());
            }
        };
        upload(type1, raw1, n1, W.data());
        if (n2) upload(type2, raw2, n2, W.data() + n1);
        DevBuf d_x((size_t)K * 4), d_x2((size_t)K * 4), d_y(((size_t)nt * R + (size_t)guard) * 4), d_res((size_t)nt * R * 4), d_tab(65536 * 2);
        HIP_CHECK(hipMemcpy(d_x.p, x, (size_t)K * 4, hipMemcpyHostToDevice));
        if (x2) HIP_CHECK(hipMemcpy(d_x2.p, x2, (size_t)K * 4, hipMemcpyHostToDevice));
        if (residual) HIP_CHECK(hipMemcpy(d_res.p, residual, (size_t)nt * R * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_y.p, 0xFF, ((size_t)nt * R + (size_t)guard) * 4));
        Tables tb;
        if (silu_table) { HIP_CHECK(hipMemcpy(d_tab.p, silu_table, 131072, hipMemcpyHostToDevice)); tb.silu = d_tab.as<__half>(); }
        ActQ A; alloc_act(A, keep, 1, (size_t)K);
        int mask = 0; for (int m = 0; m < nt; m++) mask |= act_mask_for(W[(size_t)m].type);
        if (!fuse) {
            if (prep == 1) launch_rms_quant(d_x.as<float>(), d_x2.as<float>(), 1, K, A, mask, nullptr, epi == MATVEC_EPI_REF);   // oracle-order launch: the oracle's rms mean
            else launch_silu_mul_quant(d_x.as<float>(), prep == 3 ? d_x2.as<float>() : nullptr, 1, K, A, mask, tb, nullptr);
        }
        const QWeight *Wp[4]; float *Yp[4]; const float *Rp[4];
        for (int m = 0; m < nt; m++) { Wp[m] = &W[(size_t)m]; Yp[m] = d_y.as<float>() + (size_t)m * R; Rp[m] = d_res.as<float>() + (size_t)m * R; }
        bool ok;
        if (n2) ok = launch_matvec_mixed(Wp, Yp, n1, Wp + n1, Yp + n1, n2, A, g_tune, nullptr, fuse ? prep : 0, d_x.as<float>(), d_x2.as<float>(), epi, issue_bar);
        else ok = launch_matvec_set(Wp, Yp, residual ? Rp : nullptr, n1, A, g_tune, nullptr, fuse ? prep : 0, d_x.as<float>(), d_x2.as<float>(), &tb, epi, issue_bar);
        if (!ok) { set_last_error("shape / type outside the decode mat-vec kernel's range"); return 4; }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(y, d_y.p, ((size_t)(epi == 1 ? 1 : nt) * R + (size_t)guard) * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// The batched-decode mat-vec (k_matvec_tn) as Engine::forward_batch issues it: N = 1..4 rows against n_mat equally spaced matrices (raw_w = their file bytes
// back to back), optional residual.  x: [N][n_in]; y / residual: [n_mat][N][n_out].  Returns 4 when the shape is outside the kernel's range.
// prepare = 0: the rows are quantised by a launch of their own (rms_w: normed with it there); 1: inside the mat-vec launch -- rms_norm(x_t) * rms_w, or x_t as it is.
static int test_matvec_rows_impl(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int N, const float *residual, const float *rms_w, int prepare, float *y);
int minigpt4_amd_test_matvec_rows(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int N, const float *residual, float *y) {
    return test_matvec_rows_impl(ggml_type, raw_w, n_mat, n_in, n_out, x, N, residual, nullptr, 0, y);
}
int minigpt4_amd_test_matvec_rows_prep(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int N, const float *residual, const float *rms_w, int prepare, float *y) {
    return test_matvec_rows_impl(ggml_type, raw_w, n_mat, n_in, n_out, x, N, residual, rms_w, prepare, y);
}
// bit 0: matvec_prologue_supported, bit 1: matvec_silu_pair_supported, bit 2: matvec_rows_prologue_ok -- what the engine asks before it fuses a preparation (host only)
int minigpt4_amd_test_matvec_predicates(int ggml_type, int64_t n_in) {
    if (n_in <= 0 || n_in > (1 << 30)) return -1;
    return (matvec_prologue_supported(ggml_type, (int)n_in) ? 1 : 0) | (matvec_silu_pair_supported(ggml_type, (int)n_in) ? 2 : 0) | (matvec_rows_prologue_ok(ggml_type, (int)n_in) ? 4 : 0);
}
static int test_matvec_rows_impl(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int N, const float *residual, const float *rms_w, int prepare, float *y) {
    if (!raw_w || !x || !y || n_in <= 0 || n_out <= 0 || n_mat < 1 || n_mat > 3 || N < 1 || N > 4 || !qweight_supported(ggml_type) || n_in % gt_block(ggml_type)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int K = (int)n_in, R = (int)n_out;
        QWeight plan; const size_t need = plan_qweight(ggml_type, R, K, plan, nullptr), raw_bytes = gt_nbytes(ggml_type, (size_t)R * K);
        DevBuf planes(need * (size_t)n_mat), d_raw(raw_bytes), d_x((size_t)N * K * 4), d_y((size_t)n_mat * N * R * 4), d_res((size_t)n_mat * N * R * 4);
        std::vector<QWeight> W((size_t)n_mat);
        for (int m = 0; m < n_mat; m++) {
            plan_qweight(ggml_type, R, K, W[(size_t)m], planes.as<uint8_t>() + (size_t)m * need);
            HIP_CHECK(hipMemcpy(d_raw.p, (const uint8_t *)raw_w + (size_t)m * raw_bytes, raw_bytes, hipMemcpyHostToDevice));
            if (ggml_type == GT_F16 || ggml_type == GT_F32) HIP_CHECK(hipMemcpy(planes.as<uint8_t>() + (size_t)m * need, d_raw.p, raw_bytes, hipMemcpyDeviceToDevice)); else launch_repack(d_raw.as<uint8_t>(), W[(size_t)m], nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        }
        HIP_CHECK(hipMemcpy(d_x.p, x, (size_t)N * K * 4, hipMemcpyHostToDevice));
        if (residual) HIP_CHECK(hipMemcpy(d_res.p, residual, (size_t)n_mat * N * R * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_y.p, 0xFF, (size_t)n_mat * N * R * 4));
        ActQ A; std::vector<std::unique_ptr<DevBuf>> keep; alloc_act(A, keep, (size_t)N, (size_t)K);
        DevBuf d_w((size_t)K * 4);
        if (rms_w) HIP_CHECK(hipMemcpy(d_w.p, rms_w, (size_t)K * 4, hipMemcpyHostToDevice));
        if (!prepare) launch_rms_quant(d_x.as<float>(), rms_w ? d_w.as<float>() : nullptr, N, K, A, act_mask_for(ggml_type), nullptr);
        const QWeight *Wp[3]; float *Yp[3]; const float *Rp[3];
        for (int m = 0; m < n_mat; m++) { Wp[m] = &W[(size_t)m]; Yp[m] = d_y.as<float>() + (size_t)m * N * R; Rp[m] = d_res.as<float>() + (size_t)m * N * R; }
        if (!launch_matvec_rows(Wp, Yp, residual ? Rp : nullptr, n_mat, A, N, R, g_tune, nullptr, prepare ? d_x.as<float>() : nullptr, prepare && rms_w ? d_w.as<float>() : nullptr, K)) { set_last_error("shape / type outside the multi-row mat-vec kernel's range"); return 4; }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(y, d_y.p, (size_t)n_mat * N * R * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// The batched decode's two-type launch (k_matvec_tn_mix) as Engine::forward_batch issues it for a "more bits" layer: n_a equally spaced matrices of type_a (Q4_K / Q5_K) +
// n_b of type_b (Q6_K), same shape, against N = 1..4 rows prepared by a launch of their own.  y: [n_a + n_b][N][n_out] followed by ONE GUARD ROW of n_out floats, the whole
// buffer prefilled with 0xFF bytes.  4: the launcher refuses the types / shape.
int minigpt4_amd_test_matvec_rows_mixed(int type_a, const void *raw_a, int n_a, int type_b, const void *raw_b, int n_b, int64_t n_in, int64_t n_out, const float *x, int N, float *y) {
    if (!raw_a || !raw_b || !x || !y || n_in <= 0 || n_out <= 0 || n_a < 1 || n_b < 1 || n_a + n_b > 3 || N < 1 || N > 4 || !qweight_supported(type_a) || !qweight_supported(type_b)) return 1;
    if (n_in % gt_block(type_a) || n_in % gt_block(type_b)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int K = (int)n_in, R = (int)n_out, n = n_a + n_b;
        std::vector<std::unique_ptr<DevBuf>> keep;
        std::vector<QWeight> W((size_t)n);
        auto upload = [&](int type, const void *raw, int cnt, QWeight *dst) {
            QWeight plan; const size_t need = plan_qweight(type, R, K, plan, nullptr), raw_bytes = gt_nbytes(type, (size_t)R * K);
            keep.emplace_back(new DevBuf(need * (size_t)cnt)); uint8_t *base = (uint8_t *)keep.back()->p;   // one allocation: equal spacing
            DevBuf d_raw(raw_bytes);
            for (int m = 0; m < cnt; m++) {
                plan_qweight(type, R, K, dst[m], base + (size_t)m * need);
                HIP_CHECK(hipMemcpy(d_raw.p, (const uint8_t *)raw + (size_t)m * raw_bytes, raw_bytes, hipMemcpyHostToDevice));
                if (type == GT_F16 || type == GT_F32) HIP_CHECK(hipMemcpy(base + (size_t)m * need, d_raw.p, raw_bytes, hipMemcpyDeviceToDevice)); else launch_repack(d_raw.as<uint8_t>(), dst[m], nullptr);
                HIP_CHECK(hipDeviceSynchronize());
            }
        };
        upload(type_a, raw_a, n_a, W.data());
        upload(type_b, raw_b, n_b, W.data() + n_a);
        const size_t yn = ((size_t)n * N + 1) * R;
        DevBuf d_x((size_t)N * K * 4), d_y(yn * 4);
        HIP_CHECK(hipMemcpy(d_x.p, x, (size_t)N * K * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_y.p, 0xFF, yn * 4));
        ActQ A; alloc_act(A, keep, (size_t)N, (size_t)K);
        launch_rms_quant(d_x.as<float>(), nullptr, N, K, A, act_mask_for(type_a) | act_mask_for(type_b), nullptr);
        const QWeight *Wp[3]; float *Yp[3];
        for (int m = 0; m < n; m++) { Wp[m] = &W[(size_t)m]; Yp[m] = d_y.as<float>() + (size_t)m * N * R; }
        if (!launch_matvec_rows_mixed(Wp, Yp, n_a, Wp + n_a, Yp + n_a, n_b, A, N, R, g_tune, nullptr, nullptr, nullptr, K)) { set_last_error("types / shape outside the two-type multi-row mat-vec kernel's range"); return 4; }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(y, d_y.p, yn * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// The batched decode's MFMA launch (ri_kernels.hip): n_mat equally shaped k-quant matrices (rows of raw_w back to back) as ordinary planes -> row-interleaved image -> N = 1..4
// prepared rows; y [n_mat][N][n_out].  4: the kernel refuses the shape / type.
int minigpt4_amd_test_matvec_ri(int ggml_type, const void *raw_w, int n_mat, int64_t n_in, int64_t n_out, const float *x, int N, const float *residual, const float *rms_w, float *y) {
    if (!raw_w || !x || !y || n_in <= 0 || n_out <= 0 || n_mat < 1 || n_mat > 3 || N < 1 || N > 4 || !qweight_supported(ggml_type) || n_in % gt_block(ggml_type)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int K = (int)n_in, R = (int)n_out;
        if (!ri_supported(ggml_type, R, K)) { set_last_error("type / shape outside the row-interleaved kernel's range"); return 4; }
        QWeight plan; const size_t need = plan_qweight(ggml_type, R, K, plan, nullptr), raw_bytes = gt_nbytes(ggml_type, (size_t)R * K);
        RiPlanes rplan; const size_t rneed = ri_plan(ggml_type, R, K, rplan, nullptr);
        DevBuf planes(need * (size_t)n_mat), rplanes(rneed * (size_t)n_mat), d_raw(raw_bytes), d_x((size_t)N * K * 4), d_y((size_t)n_mat * N * R * 4), d_res((size_t)n_mat * N * R * 4);
        std::vector<QWeight> W((size_t)n_mat); std::vector<RiPlanes> P((size_t)n_mat);
        for (int m = 0; m < n_mat; m++) {
            plan_qweight(ggml_type, R, K, W[(size_t)m], planes.as<uint8_t>() + (size_t)m * need);
            HIP_CHECK(hipMemcpy(d_raw.p, (const uint8_t *)raw_w + (size_t)m * raw_bytes, raw_bytes, hipMemcpyHostToDevice));
            launch_repack(d_raw.as<uint8_t>(), W[(size_t)m], nullptr);
            ri_plan(ggml_type, R, K, P[(size_t)m], rplanes.as<uint8_t>() + (size_t)m * rneed);
            launch_ri_build(W[(size_t)m], P[(size_t)m], nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        }
        HIP_CHECK(hipMemcpy(d_x.p, x, (size_t)N * K * 4, hipMemcpyHostToDevice));
        if (residual) HIP_CHECK(hipMemcpy(d_res.p, residual, (size_t)n_mat * N * R * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_y.p, 0xFF, (size_t)n_mat * N * R * 4));
        ActQ A; std::vector<std::unique_ptr<DevBuf>> keep; alloc_act(A, keep, (size_t)N, (size_t)K);
        DevBuf d_w((size_t)K * 4);
        if (rms_w) HIP_CHECK(hipMemcpy(d_w.p, rms_w, (size_t)K * 4, hipMemcpyHostToDevice));
        else launch_rms_quant(d_x.as<float>(), nullptr, N, K, A, ACT_Q8K, nullptr);                   // rms_w given: the launch norms + quantises the rows itself
        const QWeight *Wp[3]; const RiPlanes *Pp[3]; float *Yp[3]; const float *Rp[3];
        for (int m = 0; m < n_mat; m++) { Wp[m] = &W[(size_t)m]; Pp[m] = &P[(size_t)m]; Yp[m] = d_y.as<float>() + (size_t)m * N * R; Rp[m] = d_res.as<float>() + (size_t)m * N * R; }
        const LaunchTuning tune = hook_tuning();
        DevBuf d_ws(((size_t)1 << 18) * 4 + 4096);                           // K-split workspace (few groups, long K): slabs + zeroed tickets
        HIP_CHECK(hipMemset(d_ws.p, 0, ((size_t)1 << 18) * 4 + 4096));
        const RiWorkspace ws{d_ws.as<float>(), (size_t)1 << 18, reinterpret_cast<unsigned *>(d_ws.as<float>() + ((size_t)1 << 18)), 1024};
        if (!launch_matvec_ri(Wp, Pp, Yp, residual ? Rp : nullptr, n_mat, A, N, R, tune, nullptr, rms_w ? d_x.as<float>() : nullptr, rms_w ? d_w.as<float>() : nullptr, K, ws)) { set_last_error("launch_matvec_ri refused"); return 4; }
        HIP_CHECK(hipDeviceSynchronize());
        if (!launch_matvec_ri(Wp, Pp, Yp, residual ? Rp : nullptr, n_mat, A, N, R, tune, nullptr, rms_w ? d_x.as<float>() : nullptr, rms_w ? d_w.as<float>() : nullptr, K, ws)) { set_last_error("launch_matvec_ri refused"); return 4; }   // twice: the tickets must be back at zero
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(y, d_y.p, (size_t)n_mat * N * R * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// the mixed-type launch of a "more bits" layer: n_a matrices of type_a (Q4_K / Q5_K) + n_b of type_b (Q6_K), same shape -> y [n_a + n_b][N][n_out]
int minigpt4_amd_test_matvec_ri_mixed(int type_a, const void *raw_a, int n_a, int type_b, const void *raw_b, int n_b, int64_t n_in, int64_t n_out, const float *x, int N, float *y) {
    if (!raw_a || !raw_b || !x || !y || n_in <= 0 || n_out <= 0 || n_a < 1 || n_b < 1 || n_a + n_b > 3 || N < 1 || N > 4 || !qweight_supported(type_a) || !qweight_supported(type_b)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int K = (int)n_in, R = (int)n_out, n = n_a + n_b;
        if (!ri_supported(type_a, R, K) || !ri_supported(type_b, R, K)) { set_last_error("type / shape outside the row-interleaved kernel's range"); return 4; }
        std::vector<QWeight> W((size_t)n); std::vector<RiPlanes> P((size_t)n);
        std::vector<std::unique_ptr<DevBuf>> hold;
        for (int m = 0; m < n; m++) {
            const int ty = m < n_a ? type_a : type_b;
            QWeight plan; const size_t need = plan_qweight(ty, R, K, plan, nullptr), raw_bytes = gt_nbytes(ty, (size_t)R * K);
            RiPlanes rplan; const size_t rneed = ri_plan(ty, R, K, rplan, nullptr);
            hold.emplace_back(new DevBuf(need)); DevBuf &pl = *hold.back();
            hold.emplace_back(new DevBuf(rneed)); DevBuf &rp = *hold.back();
            DevBuf d_raw(raw_bytes);
            const uint8_t *src = m < n_a ? (const uint8_t *)raw_a + (size_t)m * raw_bytes : (const uint8_t *)raw_b + (size_t)(m - n_a) * raw_bytes;
            plan_qweight(ty, R, K, W[(size_t)m], pl.as<uint8_t>());
            HIP_CHECK(hipMemcpy(d_raw.p, src, raw_bytes, hipMemcpyHostToDevice));
            launch_repack(d_raw.as<uint8_t>(), W[(size_t)m], nullptr);
            ri_plan(ty, R, K, P[(size_t)m], rp.as<uint8_t>());
            launch_ri_build(W[(size_t)m], P[(size_t)m], nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        }
        DevBuf d_x((size_t)N * K * 4), d_y((size_t)n * N * R * 4);
        HIP_CHECK(hipMemcpy(d_x.p, x, (size_t)N * K * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_y.p, 0xFF, (size_t)n * N * R * 4));
        ActQ A; std::vector<std::unique_ptr<DevBuf>> keep; alloc_act(A, keep, (size_t)N, (size_t)K);
        launch_rms_quant(d_x.as<float>(), nullptr, N, K, A, ACT_Q8K, nullptr);
        const QWeight *Wa[2], *Wb[2]; const RiPlanes *Pa[2], *Pb[2]; float *Ya[2], *Yb[2];
        for (int m = 0; m < n; m++) {
            float *yo = d_y.as<float>() + (size_t)m * N * R;
            if (m < n_a) { Wa[m] = &W[(size_t)m]; Pa[m] = &P[(size_t)m]; Ya[m] = yo; } else { Wb[m - n_a] = &W[(size_t)m]; Pb[m - n_a] = &P[(size_t)m]; Yb[m - n_a] = yo; }
        }
        const LaunchTuning tune = hook_tuning();
        if (!launch_matvec_ri_mixed(Wa, Pa, Ya, n_a, Wb, Pb, Yb, n_b, A, N, R, tune, nullptr)) { set_last_error("launch_matvec_ri_mixed refused"); return 4; }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(y, d_y.p, (size_t)n * N * R * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// microseconds per launch of the row-interleaved MFMA mat-vec for one set of n_mat rows x cols matrices against N prepared rows; n_sets weight sets are rotated
int minigpt4_amd_bench_matvec_ri(int ggml_type, int rows, int cols, int n_mat, int N, int iters, int n_sets, float *us_per_launch) {
    if (!ri_supported(ggml_type, rows, cols) || n_mat < 1 || n_mat > 3 || N < 1 || N > 4 || iters < 1 || n_sets < 1) return 1;
    if (device_count_noexcept() <= 0) return 2;
    return guarded(3, [&]() -> int {
        const LaunchTuning tune = hook_tuning();
        QWeight plan; const size_t need = plan_qweight(ggml_type, rows, cols, plan, nullptr);
        RiPlanes rplan; const size_t rneed = ri_plan(ggml_type, rows, cols, rplan, nullptr);
        std::vector<std::unique_ptr<DevBuf>> keep;
        std::vector<QWeight> W((size_t)n_sets * n_mat); std::vector<RiPlanes> P((size_t)n_sets * n_mat);
        DevBuf tmp(need);
        for (size_t i = 0; i < W.size(); i++) {
            plan_qweight(ggml_type, rows, cols, W[i], tmp.as<uint8_t>());
            launch_fill_random(tmp.p, need, (unsigned)(i * 7919 + 13), nullptr);
            const size_t n = (size_t)rows * cols;
            if (ggml_type == GT_Q4_K || ggml_type == GT_Q5_K) launch_fill_u16((void *)W[i].sc, n / 256 * 16 / 2, 0x1C00, nullptr);
            if (W[i].d) launch_fill_u16((void *)W[i].d, n / 256, 0x1C00, nullptr);
            keep.emplace_back(new DevBuf(rneed));
            ri_plan(ggml_type, rows, cols, P[i], (uint8_t *)keep.back()->p);
            launch_ri_build(W[i], P[i], nullptr);
            HIP_CHECK(hipDeviceSynchronize());
        }
        ActQ A; alloc_act(A, keep, (size_t)N, (size_t)cols);
        DevBuf dx((size_t)N * cols * 4), dy((size_t)rows * 4 * 3 * N);
        { std::vector<float> hx((size_t)N * cols); for (size_t i = 0; i < hx.size(); i++) hx[i] = (float)((int)(i * 37 % 201) - 100) / 64.0f; HIP_CHECK(hipMemcpy(dx.p, hx.data(), hx.size() * 4, hipMemcpyHostToDevice)); }
        launch_rms_quant(dx.as<float>(), nullptr, N, cols, A, ACT_Q8K, nullptr);
        DevBuf d_ws(((size_t)1 << 18) * 4 + 4096);
        HIP_CHECK(hipMemset(d_ws.p, 0, ((size_t)1 << 18) * 4 + 4096));
        const RiWorkspace ws = getenv("MG4_RI_NOSPLIT") ? RiWorkspace{} : RiWorkspace{d_ws.as<float>(), (size_t)1 << 18, reinterpret_cast<unsigned *>(d_ws.as<float>() + ((size_t)1 << 18)), 1024};
        auto run = [&](int set) {
            const QWeight *Wp[3]; const RiPlanes *Pp[3]; float *Yp[3];
            for (int m = 0; m < n_mat; m++) { Wp[m] = &W[(size_t)set * n_mat + m]; Pp[m] = &P[(size_t)set * n_mat + m]; Yp[m] = dy.as<float>() + (size_t)m * rows * N; }
            if (!launch_matvec_ri(Wp, Pp, Yp, nullptr, n_mat, A, N, rows, tune, nullptr, nullptr, nullptr, 0, ws)) throw HipError{hipErrorInvalidValue, "launch_matvec_ri refused", __FILE__, __LINE__};
        };
        for (int i = 0; i < std::min(n_sets, 4); i++) run(i);
        HIP_CHECK(hipDeviceSynchronize());
        float ms = 0;
        timed(&ms, [&] { for (int i = 0; i < iters; i++) run(i % n_sets); return true; });
        if (us_per_launch) *us_per_launch = ms * 1e3f / (float)iters;
        return 0;
    });
}

int minigpt4_amd_test_quantize(const float *x, const float *rms_w, int64_t N, int64_t K, int8_t *q8k, float *dk, int16_t *bsums, int8_t *q80, float *d0) {
    if (!x || N <= 0 || K <= 0 || K % 256) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        DevBuf d_x((size_t)(N * K) * 4), d_w((size_t)K * 4);
        HIP_CHECK(hipMemcpy(d_x.p, x, (size_t)(N * K) * 4, hipMemcpyHostToDevice));
        if (rms_w) HIP_CHECK(hipMemcpy(d_w.p, rms_w, (size_t)K * 4, hipMemcpyHostToDevice));
        ActQ A; std::vector<std::unique_ptr<DevBuf>> keep; alloc_act(A, keep, (size_t)N, (size_t)K);
        launch_rms_quant(d_x.as<float>(), rms_w ? d_w.as<float>() : nullptr, (int)N, (int)K, A, ACT_Q8K | ACT_Q80, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (q8k) HIP_CHECK(hipMemcpy(q8k, A.q8k, (size_t)(N * K), hipMemcpyDeviceToHost));
        if (dk) HIP_CHECK(hipMemcpy(dk, A.dk, (size_t)(N * K / 256) * 4, hipMemcpyDeviceToHost));
        if (bsums) HIP_CHECK(hipMemcpy(bsums, A.bsk, (size_t)(N * K / 16) * 2, hipMemcpyDeviceToHost));
        if (q80) HIP_CHECK(hipMemcpy(q80, A.q80, (size_t)(N * K), hipMemcpyDeviceToHost));
        if (d0) HIP_CHECK(hipMemcpy(d0, A.d0, (size_t)(N * K / 32) * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

}  // extern "C"

// ---- the activation-preparation kernels and the consumers of a deferred split-K combine, one launch each (tests/test_gpu_act_prepare.py) ----
namespace {
constexpr int AP_PLANES = 13, AP_MAX_N = 4096, AP_MAX_K = 1 << 16, AP_MAX_KS = 16;
// An ActQ whose thirteen planes are N + 1 rows of device memory each, prefilled with 0xFF bytes (row N: the guard row).  planes: 1 bsq, 2 bs16, 4 q16 exist.
struct GuardedAct {
    ActQ A; std::vector<std::unique_ptr<DevBuf>> keep; size_t bytes[AP_PLANES]; void *dev[AP_PLANES];
    GuardedAct(size_t N, size_t K, int planes) {
        const size_t row[AP_PLANES] = {K, K / 256 * 4, K / 16 * 2, K / 256 * 16, K / 256 * 32, K * 2, K, K / 32 * 4, K / 32 * 4, K / 32 * 4, K / 32 * 4, K * 2, K * 4};
        for (int i = 0; i < AP_PLANES; i++) {
            bytes[i] = (N + 1) * row[i];
            keep.emplace_back(new DevBuf(bytes[i] + 256)); dev[i] = keep.back()->p;
            HIP_CHECK(hipMemset(dev[i], 0xFF, bytes[i] + 256));
        }
        A.q8k = (int8_t *)dev[0]; A.dk = (float *)dev[1]; A.bsk = (int16_t *)dev[2];
        A.bsq = (planes & 1) ? (int8_t *)dev[3] : nullptr; A.bs16 = (planes & 2) ? (__half *)dev[4] : nullptr; A.q16 = (planes & 4) ? (__half *)dev[5] : nullptr;
        A.q80 = (int8_t *)dev[6]; A.d0 = (float *)dev[7]; A.d1 = (float *)dev[8]; A.s1 = (float *)dev[9]; A.sum0 = (int *)dev[10]; A.xh = (__half *)dev[11]; A.xf = (float *)dev[12];
    }
    void copy_back(void *const out[AP_PLANES]) { for (int i = 0; i < AP_PLANES; i++) if (out[i] && bytes[i]) HIP_CHECK(hipMemcpy(out[i], dev[i], bytes[i], hipMemcpyDeviceToHost)); }
};
// what every kernel that ends in quant_emit4 needs of (N, K, mask): float4 loads, whole Q8_K / Q8_0 blocks
bool prepare_shape_ok(int64_t N, int64_t K, int mask, int planes) {
    if (N < 1 || N > AP_MAX_N || K < 4 || K > AP_MAX_K || K % 4 || mask < 1 || mask > 15 || planes < 0 || planes > 7 || ((planes & 2) && !(planes & 1))) return false;
    return !((mask & ACT_Q8K) && K % 256) && !((mask & ACT_Q80) && K % 32);
}
void ap_upload(DevBuf &d, const float *src, size_t n) { HIP_CHECK(hipMemcpy(d.p, src, n * 4, hipMemcpyHostToDevice)); }
// slab counts of a SlabSrc's matrices -> in which slab of the back-to-back host array each matrix begins, and how many slabs there are in all; a matrix with count 1 is
// in place and has no slab, which only the matrices from first_in_place_ok on may be
bool slab_layout(const int32_t *mks, int n, int first_in_place_ok, size_t begin[3], size_t &total) {
    total = 0;
    for (int i = 0; i < n; i++) {
        if (mks[i] < 1 || mks[i] > AP_MAX_KS || (mks[i] == 1 && i < first_in_place_ok)) return false;
        begin[i] = total;
        if (mks[i] > 1) total += (size_t)mks[i];
    }
    return true;
}
}  // namespace

extern "C" {

int minigpt4_amd_test_prepare(int launcher, const float *x, const float *second, int64_t N, int64_t K, int mask, int planes, int sequential_sum, const unsigned short *silu_table,
                              int8_t *q8k, float *dk, int16_t *bsk, int8_t *bsq, unsigned short *bs16, unsigned short *q16, int8_t *q80, float *d0, float *d1, float *s1,
                              int32_t *sum0, unsigned short *xh, float *xf) {
    if (!x || (launcher != 0 && launcher != 1) || !prepare_shape_ok(N, K, mask, planes)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t nk = (size_t)(N * K), n2 = launcher == 0 ? (size_t)K : nk;
        DevBuf dx(nk * 4), d2(n2 * 4), dtab(65536 * 2);
        ap_upload(dx, x, nk);
        if (second) ap_upload(d2, second, n2);
        Tables tb;
        if (silu_table) { HIP_CHECK(hipMemcpy(dtab.p, silu_table, 131072, hipMemcpyHostToDevice)); tb.silu = dtab.as<__half>(); }
        GuardedAct G((size_t)N, (size_t)K, planes);
        if (launcher == 0) launch_rms_quant(dx.as<float>(), second ? d2.as<float>() : nullptr, (int)N, (int)K, G.A, mask, nullptr, sequential_sum != 0);
        else launch_silu_mul_quant(dx.as<float>(), second ? d2.as<float>() : nullptr, (int)N, (int)K, G.A, mask, tb, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        void *const out[AP_PLANES] = {q8k, dk, bsk, bsq, bs16, q16, q80, d0, d1, s1, sum0, xh, xf};
        G.copy_back(out);
        return 0;
    });
}

int minigpt4_amd_test_prepare_slabs(int launcher, const float *slabs, int ks, int64_t stride, const float *residual, int in_place, const float *w, int64_t N, int64_t K, int mask,
                                    int planes, const unsigned short *silu_table, float *x_out, int8_t *q8k, float *dk, int16_t *bsk, int8_t *bsq, unsigned short *bs16,
                                    unsigned short *q16, int8_t *q80, float *d0, float *d1, float *s1, int32_t *sum0, unsigned short *xh, float *xf) {
    if (!slabs || (launcher != 0 && launcher != 1) || !prepare_shape_ok(N, K, mask, planes) || ks < 2 || ks > AP_MAX_KS || stride < N * K || stride % 4 || stride > ((int64_t)1 << 26)) return 1;
    if (launcher == 0 ? (!w || !x_out || (in_place && !residual)) : (!silu_table || residual || in_place || w || x_out)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t nk = (size_t)(N * K), gk = nk + (size_t)K, ns = (size_t)(launcher == 0 ? 1 : 2) * (size_t)ks * (size_t)stride;
        DevBuf ds(ns * 4), dres(nk * 4), dw((size_t)K * 4), dxo(gk * 4), dtab(65536 * 2);
        ap_upload(ds, slabs, ns);
        HIP_CHECK(hipMemset(dxo.p, 0xFF, gk * 4));
        if (residual) ap_upload(in_place ? dxo : dres, residual, nk);
        if (w) ap_upload(dw, w, (size_t)K);
        Tables tb;
        if (silu_table) { HIP_CHECK(hipMemcpy(dtab.p, silu_table, 131072, hipMemcpyHostToDevice)); tb.silu = dtab.as<__half>(); }
        GuardedAct G((size_t)N, (size_t)K, planes);
        SlabSrc S; S.ws = ds.as<float>(); S.ks = ks; S.stride = (long long)stride; S.n = launcher == 0 ? 1 : 2;
        for (int m = 0; m < S.n; m++) { S.mbase[m] = S.ws + (size_t)m * ks * (size_t)stride; S.mks[m] = ks; }
        if (launcher == 0) {
            S.y[0] = dxo.as<float>(); S.res[0] = residual ? (in_place ? dxo.as<float>() : dres.as<float>()) : nullptr;
            launch_rms_quant_slabs(S, dw.as<float>(), (int)N, (int)K, G.A, mask, nullptr);
        } else launch_silu_mul_quant_slabs(S, (int)N, (int)K, G.A, mask, tb, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (x_out) HIP_CHECK(hipMemcpy(x_out, dxo.p, gk * 4, hipMemcpyDeviceToHost));
        void *const out[AP_PLANES] = {q8k, dk, bsk, bsq, bs16, q16, q80, d0, d1, s1, sum0, xh, xf};
        G.copy_back(out);
        return 0;
    });
}

int minigpt4_amd_test_slab_flush(int n, int mixed, const int32_t *mks, const float *slabs, int64_t stride, const float *residual, int residual_mask, float *y) {
    size_t begin[3] = {0, 0, 0}, total = 0;
    if (!mks || !slabs || !y || n < 1 || n > 3 || stride < 4 || stride % 4 || stride > ((int64_t)1 << 26) || residual_mask < 0 || residual_mask >= (1 << n) || (residual_mask && !residual)) return 1;
    if (!slab_layout(mks, n, mixed ? 1 : n, begin, total)) return 1;
    if (!mixed) for (int i = 1; i < n; i++) if (mks[i] != mks[0]) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t st = (size_t)stride, ny = (size_t)(n + 1) * st;
        DevBuf ds(total * st * 4), dres((size_t)n * st * 4), dy(ny * 4);
        ap_upload(ds, slabs, total * st);
        if (residual) ap_upload(dres, residual, (size_t)n * st);
        HIP_CHECK(hipMemset(dy.p, 0xFF, ny * 4));
        SlabSrc S; S.ws = ds.as<float>(); S.ks = mks[0]; S.stride = (long long)stride; S.n = n; S.mixed = mixed != 0;
        for (int i = 0; i < n; i++) {
            S.y[i] = dy.as<float>() + (size_t)i * st;
            S.res[i] = (residual_mask >> i & 1) ? dres.as<float>() + (size_t)i * st : nullptr;
            S.mks[i] = mks[i];
            if (mks[i] == 1) { S.mbase[i] = S.y[i]; HIP_CHECK(hipMemcpy(S.y[i], y + (size_t)i * st, st * 4, hipMemcpyHostToDevice)); }   // already in place
            else S.mbase[i] = S.ws + begin[i] * st;
        }
        launch_slab_flush(S, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(y, dy.p, ny * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

int minigpt4_amd_test_rope_kv_slabs(int n_head, int hd, int n_ctx, int N, int pos0, const int32_t *mks, const float *slabs, int64_t stride, const float *v_in_place, float *q_out,
                                    uint16_t *kc, uint16_t *vc) {
    size_t begin[3] = {0, 0, 0}, total = 0;
    if (!mks || !slabs || !q_out || !kc || !vc || n_head < 1 || n_head > 256 || hd < 2 || hd > 256 || hd % 2 || N < 1 || N > AP_MAX_N || pos0 < 0 || n_ctx < 1 || n_ctx > (1 << 16) ||
        (int64_t)pos0 + N > n_ctx || stride < (int64_t)N * n_head * hd || stride % 4 || stride > ((int64_t)1 << 26)) return 1;
    if (!slab_layout(mks, 3, 2, begin, total) || (mks[2] == 1) != (v_in_place != nullptr)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t E = (size_t)n_head * hd, NE = (size_t)N * E, st = (size_t)stride, cache = (size_t)n_ctx * E;
        std::vector<float> c, sn;
        rope_tables(n_ctx, hd, c, sn);
        DevBuf dc(c.size() * 4), dsn(sn.size() * 4), ds(total * st * 4), dv(NE * 4), dq((NE + E) * 4), dkc(cache * 2), dvc(cache * 2), dnp(4);
        HIP_CHECK(hipMemcpy(dc.p, c.data(), c.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dsn.p, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
        ap_upload(ds, slabs, total * st);
        if (v_in_place) ap_upload(dv, v_in_place, NE);
        HIP_CHECK(hipMemcpy(dnp.p, &pos0, 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dq.p, 0xFF, (NE + E) * 4)); HIP_CHECK(hipMemset(dkc.p, 0, cache * 2)); HIP_CHECK(hipMemset(dvc.p, 0, cache * 2));
        SlabSrc S; S.ws = ds.as<float>(); S.ks = mks[0]; S.stride = (long long)stride; S.n = 3; S.mixed = mks[2] != mks[0];
        S.y[0] = dq.as<float>(); S.y[2] = dv.as<float>();
        for (int i = 0; i < 3; i++) { S.mks[i] = mks[i]; S.mbase[i] = mks[i] == 1 ? dv.as<float>() : S.ws + begin[i] * st; }
        launch_rope_kv_slabs(S, N, n_head, hd, dnp.as<int>(), dc.as<float>(), dsn.as<float>(), dkc.as<__half>(), dvc.as<__half>(), nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(q_out, dq.p, (NE + E) * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(kc, dkc.p, cache * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(vc, dvc.p, cache * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}

// The embedding gather (k_get_rows / dequant_elem) alone: one launch_get_rows over a raw table [n_rows][K] exactly as a model file stores it (Q3_K: re-encoded as Q6_K first,
// as the engine's load path does).  out [N + 1][K]: prefilled with 0xFF bytes, row N is a guard row; a token of -1 leaves its row at the fill.
int minigpt4_amd_test_get_rows(int ggml_type, const void *raw_table, int n_rows, int64_t K, const int32_t *tokens, int N, float *out) {
    if (!raw_table || !tokens || !out || n_rows < 1 || n_rows > (1 << 20) || K < 1 || K > (1 << 20) || N < 1 || N > (1 << 16)) return 1;
    if (ggml_type != GT_Q3_K && !qweight_supported(ggml_type)) return 1;
    if (K % gt_block(ggml_type)) return 1;
    for (int t = 0; t < N; t++) if (tokens[t] < -1 || tokens[t] >= n_rows) return 1;
    if (ggml_type == GT_Q3_K) {
        const size_t nb = (size_t)(K / 256) * (size_t)n_rows;
        std::vector<uint8_t> q6(nb * 210);
        q3k_to_q6k(static_cast<const uint8_t *>(raw_table), q6.data(), nb);
        return minigpt4_amd_test_get_rows(GT_Q6_K, q6.data(), n_rows, K, tokens, N, out);
    }
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t raw_bytes = gt_nbytes(ggml_type, (size_t)K) * (size_t)n_rows, on = ((size_t)N + 1) * (size_t)K;
        DevBuf d_raw(raw_bytes), d_tok((size_t)N * 4), d_out(on * 4);
        HIP_CHECK(hipMemcpy(d_raw.p, raw_table, raw_bytes, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_tok.p, tokens, (size_t)N * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_out.p, 0xFF, on * 4));
        launch_get_rows(ggml_type, d_raw.as<uint8_t>(), (int)K, d_tok.as<int>(), N, d_out.as<float>(), nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, d_out.p, on * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// table: the GELU table the epilogue gathers from (65536 fp16 bit patterns, uploaded); NULL with gelu set: Tables::gelu stays null -- the computed arm, as Engine::tabs_vis_ passes it
static int test_gemm_impl(const float *A, const float *W, const float *bias, int M, int N, int K, int gelu, float *C, bool skinny, const unsigned short *table);
int minigpt4_amd_test_gemm_f16(const float *A, const float *W, const float *bias, int M, int N, int K, int gelu, float *C) { return test_gemm_impl(A, W, bias, M, N, K, gelu, C, false, gelu ? host_gelu_table().data() : nullptr); }
int minigpt4_amd_test_gemm_f16_skinny(const float *A, const float *W, const float *bias, int M, int N, int K, int gelu, float *C) { return test_gemm_impl(A, W, bias, M, N, K, gelu, C, true, gelu ? host_gelu_table().data() : nullptr); }
int minigpt4_amd_test_gemm_f16_ex(const float *A, const float *W, const float *bias, int M, int N, int K, int gelu, int skinny, const unsigned short *gelu_table, float *C) { return test_gemm_impl(A, W, bias, M, N, K, gelu, C, skinny != 0, gelu_table); }
static int test_gemm_impl(const float *A, const float *W, const float *bias, int M, int N, int K, int gelu, float *C, bool skinny, const unsigned short *table) {
    if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0 || K % 16) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        DevBuf dA((size_t)M * K * 4), dW((size_t)N * K * 4), dAh((size_t)M * K * 2), dWh((size_t)N * K * 2), dC((size_t)M * N * 4), db((size_t)N * 4), dtab(65536 * 2);
        HIP_CHECK(hipMemcpy(dA.p, A, (size_t)M * K * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dW.p, W, (size_t)N * K * 4, hipMemcpyHostToDevice));
        if (bias) HIP_CHECK(hipMemcpy(db.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
        Tables tb;
        if (gelu && table) { HIP_CHECK(hipMemcpy(dtab.p, table, 131072, hipMemcpyHostToDevice)); tb.gelu = dtab.as<__half>(); }
        launch_f32_to_f16(dA.as<float>(), dAh.as<__half>(), (size_t)M * K, nullptr); launch_f32_to_f16(dW.as<float>(), dWh.as<__half>(), (size_t)N * K, nullptr);
        if (skinny) { if (!launch_gemm_f16_skinny(dAh.as<__half>(), K, dWh.as<__half>(), K, M, N, K, bias ? db.as<float>() : nullptr, nullptr, gelu != 0, tb, dC.as<float>(), nullptr, N, nullptr)) return 4; }
        else launch_gemm_f16(dAh.as<__half>(), K, dWh.as<__half>(), K, M, N, K, bias ? db.as<float>() : nullptr, nullptr, gelu != 0, tb, dC.as<float>(), nullptr, N, g_tune, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(C, dC.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// ---- the image encoder's kernels BETWEEN its GEMMs, one launch each (tests/test_gpu_vision_kernels.py).  Common form: arguments checked before a device is touched (1);
// every output buffer is prefilled with 0xFF bytes and carries one guard row past `rows`, copied back with the rows; a launcher's host-side throw arrives as 3 through guarded().
static constexpr int VK_MAX_ROWS = 4096, VK_MAX_N = 1 << 16;     // sanity caps of the hooks' allocations, far above every launcher's own limit
static void upload_f32(DevBuf &d, const float *src, size_t n) { HIP_CHECK(hipMemcpy(d.p, src, n * 4, hipMemcpyHostToDevice)); }

// launch_layernorm: x [rows][n], w [n], b [n] or NULL -> out [rows + 1][n] fp32 and / or out_h [rows + 1][n] fp16 bits (either may be NULL, not both)
int minigpt4_amd_test_layernorm(const float *x, const float *w, const float *b, int rows, int n, int sequential_sums, float *out, unsigned short *out_h) {
    if (!x || !w || (!out && !out_h) || rows < 1 || rows > VK_MAX_ROWS || n < 1 || n > VK_MAX_N) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t rn = (size_t)rows * n, gn = rn + (size_t)n;
        DevBuf dx(rn * 4), dw((size_t)n * 4), db((size_t)n * 4), dout(gn * 4), douth(gn * 2);
        upload_f32(dx, x, rn); upload_f32(dw, w, (size_t)n);
        if (b) upload_f32(db, b, (size_t)n);
        HIP_CHECK(hipMemset(dout.p, 0xFF, gn * 4)); HIP_CHECK(hipMemset(douth.p, 0xFF, gn * 2));
        launch_layernorm(dx.as<float>(), dw.as<float>(), b ? db.as<float>() : nullptr, rows, n, out ? dout.as<float>() : nullptr, out_h ? douth.as<__half>() : nullptr, nullptr, sequential_sums != 0);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (out) HIP_CHECK(hipMemcpy(out, dout.p, gn * 4, hipMemcpyDeviceToHost));
        if (out_h) HIP_CHECK(hipMemcpy(out_h, douth.p, gn * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}

// launch_splitk_reduce_ln: slabs = n_slabs x slab_stride floats (slab z's row r at z * slab_stride + r * n; slab_stride >= rows * n, the caller fills the padding);
// in_place: ONE device buffer is both `residual` and `x_out` (the ViT blocks' call).  x_out / ln_out [rows + 1][n] fp32, ln_out_h [rows + 1][n] fp16 bits
int minigpt4_amd_test_splitk_reduce_ln(const float *slabs, int n_slabs, int64_t slab_stride, const float *bias, const float *residual, int in_place, int rows, int n, const float *ln_w,
                                       const float *ln_b, float *x_out, float *ln_out, unsigned short *ln_out_h) {
    if (!slabs || n_slabs < 1 || n_slabs > 64 || rows < 1 || rows > VK_MAX_ROWS || n < 1 || n > VK_MAX_N || slab_stride < (int64_t)rows * n || slab_stride > ((int64_t)1 << 28)) return 1;
    if ((!x_out && !ln_out && !ln_out_h) || (!ln_w && (ln_b || ln_out || ln_out_h)) || (ln_w && !ln_out && !ln_out_h) || (in_place && (!residual || !x_out))) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t rn = (size_t)rows * n, gn = rn + (size_t)n, sn = (size_t)n_slabs * (size_t)slab_stride;
        DevBuf ds(sn * 4), dbias((size_t)n * 4), dres(rn * 4), dw((size_t)n * 4), db((size_t)n * 4), dx(gn * 4), dln(gn * 4), dlnh(gn * 2);
        upload_f32(ds, slabs, sn);
        if (bias) upload_f32(dbias, bias, (size_t)n);
        if (ln_w) upload_f32(dw, ln_w, (size_t)n);
        if (ln_b) upload_f32(db, ln_b, (size_t)n);
        HIP_CHECK(hipMemset(dx.p, 0xFF, gn * 4)); HIP_CHECK(hipMemset(dln.p, 0xFF, gn * 4)); HIP_CHECK(hipMemset(dlnh.p, 0xFF, gn * 2));
        if (residual) upload_f32(in_place ? dx : dres, residual, rn);
        const float *res = residual ? (in_place ? dx.as<float>() : dres.as<float>()) : nullptr;
        launch_splitk_reduce_ln(ds.as<float>(), n_slabs, (size_t)slab_stride, bias ? dbias.as<float>() : nullptr, res, rows, n, x_out ? dx.as<float>() : nullptr, ln_w ? dw.as<float>() : nullptr,
                                ln_b ? db.as<float>() : nullptr, ln_out ? dln.as<float>() : nullptr, ln_out_h ? dlnh.as<__half>() : nullptr, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (x_out) HIP_CHECK(hipMemcpy(x_out, dx.p, gn * 4, hipMemcpyDeviceToHost));
        if (ln_out) HIP_CHECK(hipMemcpy(ln_out, dln.p, gn * 4, hipMemcpyDeviceToHost));
        if (ln_out_h) HIP_CHECK(hipMemcpy(ln_out_h, dlnh.p, gn * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}

// The split-K forms of the fp16 GEMM: raw fp32 partial sums, slab z = A[:, cols of slice z] . W[:, the same]^T.  Operands as test_gemm_impl (fp32 on the host, rounded to fp16
// on the device).  skinny == 0: slices = gemm_split_slices(K, slices_wanted) as Engine::encode computes it, then launch_gemm_f16_splitk (64x64 tiles, or the ring tiles from
// 384 rows on); skinny != 0: launch_gemm_f16_skinny_splitk with slices_wanted as given -- 4, nothing launched, when it refuses.  slabs_out: room for slices_wanted slabs
// [M][N]; the first *slices_used_out are written, and only on success
int minigpt4_amd_test_gemm_f16_splitk(const float *A, const float *W, int M, int N, int K, int slices_wanted, int skinny, float *slabs_out, int *slices_used_out) {
    if (!A || !W || !slabs_out || !slices_used_out || M <= 0 || M > VK_MAX_ROWS || N <= 0 || N > VK_MAX_N || K <= 0 || K > VK_MAX_N || K % 16 || slices_wanted < 1 || slices_wanted > 64) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int slices = skinny ? slices_wanted : gemm_split_slices(K, slices_wanted);
        const size_t mn = (size_t)M * N, sn = (size_t)slices * mn + (size_t)N;           // + one guard row (never copied back: the descriptors' bounds end at the slab)
        DevBuf dA((size_t)M * K * 4), dW((size_t)N * K * 4), dAh((size_t)M * K * 2), dWh((size_t)N * K * 2), dS(sn * 4);
        upload_f32(dA, A, (size_t)M * K); upload_f32(dW, W, (size_t)N * K);
        HIP_CHECK(hipMemset(dS.p, 0xFF, sn * 4));
        launch_f32_to_f16(dA.as<float>(), dAh.as<__half>(), (size_t)M * K, nullptr); launch_f32_to_f16(dW.as<float>(), dWh.as<__half>(), (size_t)N * K, nullptr);
        if (skinny) { if (!launch_gemm_f16_skinny_splitk(dAh.as<__half>(), K, dWh.as<__half>(), K, M, N, K, slices, dS.as<float>(), mn, N, nullptr)) { HIP_CHECK(hipDeviceSynchronize()); set_last_error("launch_gemm_f16_skinny_splitk refused"); return 4; } }
        else launch_gemm_f16_splitk(dAh.as<__half>(), K, dWh.as<__half>(), K, M, N, K, slices, dS.as<float>(), mn, N, g_tune, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(slabs_out, dS.p, (size_t)slices * mn * 4, hipMemcpyDeviceToHost));
        *slices_used_out = slices;
        return 0;
    });
}

// launch_gemm_f16_head_major with N = 3 * D: out = [3 * D floats of guard][3][D / hd][M][hd][3 * D floats of guard], all of it copied back (the launcher's throw for
// D % hd != 0 arrives as 3)
int minigpt4_amd_test_gemm_f16_head_major(const float *A, const float *W, const float *bias, int M, int D, int hd, int K, float *out) {
    if (!A || !W || !out || M <= 0 || M > VK_MAX_ROWS || D <= 0 || 3 * (int64_t)D > VK_MAX_N || hd <= 0 || K <= 0 || K > VK_MAX_N || K % 16) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int N = 3 * D;
        const size_t mn = (size_t)M * N, gn = mn + 2 * (size_t)N;
        DevBuf dA((size_t)M * K * 4), dW((size_t)N * K * 4), dAh((size_t)M * K * 2), dWh((size_t)N * K * 2), dC(gn * 4), db((size_t)N * 4);
        upload_f32(dA, A, (size_t)M * K); upload_f32(dW, W, (size_t)N * K);
        if (bias) upload_f32(db, bias, (size_t)N);
        HIP_CHECK(hipMemset(dC.p, 0xFF, gn * 4));
        launch_f32_to_f16(dA.as<float>(), dAh.as<__half>(), (size_t)M * K, nullptr); launch_f32_to_f16(dW.as<float>(), dWh.as<__half>(), (size_t)N * K, nullptr);
        Tables tb;
        launch_gemm_f16_head_major(dAh.as<__half>(), K, dWh.as<__half>(), K, M, N, K, bias ? db.as<float>() : nullptr, tb, dC.as<float>() + N, D, hd, g_tune, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, dC.p, gn * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// launch_im2col: image [batch][3][224][224] fp32 -> patches [batch * 256 + 1][ldp] fp16 bits
int minigpt4_amd_test_im2col(const float *image, int batch, int ldp, unsigned short *patches) {
    if (!image || !patches || batch < 1 || batch > 16 || ldp < 588 || ldp > 4096) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t ni = (size_t)batch * 3 * 224 * 224, np = ((size_t)batch * 256 + 1) * ldp;
        DevBuf di(ni * 4), dp(np * 2);
        upload_f32(di, image, ni);
        HIP_CHECK(hipMemset(dp.p, 0xFF, np * 2));
        launch_im2col(di.as<float>(), dp.as<__half>(), ldp, nullptr, batch);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(patches, dp.p, np * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}

// launch_assemble_embeddings: cls [D], pe [batch * 256][D], pos [257][D] -> x [batch * 257 + 1][D]
int minigpt4_amd_test_assemble(const float *cls, const float *pe, const float *pos, int batch, int D, float *x) {
    if (!cls || !pe || !pos || !x || batch < 1 || batch > 16 || D < 1 || D > VK_MAX_N) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t npe = (size_t)batch * 256 * D, npos = (size_t)257 * D, nx = ((size_t)batch * 257 + 1) * D;
        DevBuf dc((size_t)D * 4), dpe(npe * 4), dpos(npos * 4), dx(nx * 4);
        upload_f32(dc, cls, (size_t)D); upload_f32(dpe, pe, npe); upload_f32(dpos, pos, npos);
        HIP_CHECK(hipMemset(dx.p, 0xFF, nx * 4));
        launch_assemble_embeddings(dc.as<float>(), dpe.as<float>(), dpos.as<float>(), D, dx.as<float>(), nullptr, batch);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(x, dx.p, nx * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}

// launch_lin_epilogue: y / residual [rows][n], bias [n]; gelu_table (65536 fp16 bit patterns) non-NULL = the GELU step, gathered from it (this launch has no computed arm:
// the engine always hands it the tables).  out [rows + 1][n] fp32 and / or out_h [rows + 1][n] fp16 bits
int minigpt4_amd_test_lin_epilogue(const float *y, const float *bias, const float *residual, const unsigned short *gelu_table, int rows, int n, float *out, unsigned short *out_h) {
    if (!y || (!out && !out_h) || rows < 1 || rows > VK_MAX_ROWS || n < 1 || n > VK_MAX_N) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t rn = (size_t)rows * n, gn = rn + (size_t)n;
        DevBuf dy(rn * 4), dbias((size_t)n * 4), dres(rn * 4), dtab(65536 * 2), dout(gn * 4), douth(gn * 2);
        upload_f32(dy, y, rn);
        if (bias) upload_f32(dbias, bias, (size_t)n);
        if (residual) upload_f32(dres, residual, rn);
        Tables tb;
        if (gelu_table) { HIP_CHECK(hipMemcpy(dtab.p, gelu_table, 131072, hipMemcpyHostToDevice)); tb.gelu = dtab.as<__half>(); }
        HIP_CHECK(hipMemset(dout.p, 0xFF, gn * 4)); HIP_CHECK(hipMemset(douth.p, 0xFF, gn * 2));
        launch_lin_epilogue(dy.as<float>(), bias ? dbias.as<float>() : nullptr, residual ? dres.as<float>() : nullptr, gelu_table != nullptr, tb, rows, n, out ? dout.as<float>() : nullptr,
                            out_h ? douth.as<__half>() : nullptr, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        if (out) HIP_CHECK(hipMemcpy(out, dout.p, gn * 4, hipMemcpyDeviceToHost));
        if (out_h) HIP_CHECK(hipMemcpy(out_h, douth.p, gn * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}

// Micro-benchmark of the fp16 GEMM of the image path on synthetic operands (tools/timeline_gemm.py): `iters` launches of C[M][N] = A[M][K] . W[N][K]^T, cycling through
// `n_sets` weight matrices so that the Infinity Cache cannot serve repeats (as in the encoder, where every block has its own weights).  flags: 1 = GELU epilogue,
// 2 = residual epilogue, 4 = fp16 output as well.  variant 0 = launch_gemm_f16 (the dispatcher: 128x128 tiles from M = 512, 64x64 below), 1 = the skinny-M kernel,
// 2 = split K in `slices` + k_splitk_reduce_ln (the ViT's fc2 form; `slices` in bits 8.. of `variant`).
int minigpt4_amd_bench_gemm_f16(int M, int N, int K, int flags, int variant, int iters, int n_sets, float *us_per_launch) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 16 || iters < 1 || n_sets < 1) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int slices = std::max(1, (variant >> 8) & 255), sk_arm = variant >> 16; variant &= 255;
        DevBuf dA((size_t)M * K * 2), dC((size_t)M * N * 4), dCh((size_t)M * N * 2), dR((size_t)M * N * 4), db((size_t)N * 4), dtab(65536 * 2), dslab((size_t)std::max(slices, 8) * M * N * 4), dln((size_t)N * 4);
        std::vector<std::unique_ptr<DevBuf>> W;
        for (int i = 0; i < n_sets; i++) { W.emplace_back(new DevBuf((size_t)N * K * 2)); launch_fill_u16(W.back()->p, (size_t)N * K, (unsigned short)(0x2E66 + i), nullptr); }
        launch_fill_u16(dA.p, (size_t)M * K, 0x3266, nullptr); launch_fill_u16(dtab.p, 65536, 0x3800, nullptr);
        HIP_CHECK(hipMemset(dR.p, 0, (size_t)M * N * 4)); HIP_CHECK(hipMemset(db.p, 0, (size_t)N * 4)); HIP_CHECK(hipMemset(dln.p, 0, (size_t)N * 4));
        Tables tb; tb.gelu = dtab.as<__half>();
        const bool gelu = flags & 1, res = flags & 2;
        auto run = [&](int set) -> bool {
            const __half *Wh = W[(size_t)set]->as<__half>();
            if (variant == 1) return launch_gemm_f16_skinny(dA.as<__half>(), K, Wh, K, M, N, K, db.as<float>(), res ? dR.as<float>() : nullptr, gelu, tb, dC.as<float>(), (flags & 4) ? dCh.as<__half>() : nullptr, N, nullptr);
            if (variant == 2) {
                int sl = gemm_split_slices(K, slices);
                if (sk_arm) { sl = slices; if (!launch_gemm_f16_splitk_arm(sk_arm, dA.as<__half>(), K, Wh, K, M, N, K, sl, dslab.as<float>(), (size_t)M * N, N, g_tune, nullptr)) return false; }
                else launch_gemm_f16_splitk(dA.as<__half>(), K, Wh, K, M, N, K, sl, dslab.as<float>(), (size_t)M * N, N, g_tune, nullptr);
                if (N > 2048) launch_slab_reduce(dslab.as<float>(), sl, (long long)M * N, dR.as<float>(), dC.as<float>(), (size_t)M * N, nullptr);   // the language model's combine
                else launch_splitk_reduce_ln(dslab.as<float>(), sl, (size_t)M * N, db.as<float>(), dR.as<float>(), M, N, dC.as<float>(), dln.as<float>(), dln.as<float>(), nullptr, dCh.as<__half>(), nullptr);
                return true;
            }
            if (variant >= 101 && variant <= 103) {   // the F16 language model's set launch (n = variant - 100 equally spaced matrices of N columns each; wo / w2: n = 1 with a residual)
                const int n = variant - 100;
                const __half *Wp[3]; float *Yp[3]; const float *Rp[3];
                for (int m = 0; m < n; m++) { Wp[m] = Wh + (size_t)m * (N / n) * K; Yp[m] = dC.as<float>() + (size_t)m * M * (N / n); Rp[m] = dR.as<float>() + (size_t)m * M * (N / n); }
                return launch_gemm_f16_set(dA.as<__half>(), K, Wp, n, M, N / n, K, Yp, res ? Rp : nullptr, N / n, dslab.as<float>(), (size_t)8 * M * N, g_tune, nullptr);
            }
            if (variant >= 3 && variant < 100) return launch_gemm_f16_arm(variant, dA.as<__half>(), K, Wh, K, M, N, K, db.as<float>(), res ? dR.as<float>() : nullptr, gelu, tb, dC.as<float>(), (flags & 4) ? dCh.as<__half>() : nullptr, N, g_tune, nullptr);
            launch_gemm_f16(dA.as<__half>(), K, Wh, K, M, N, K, db.as<float>(), res ? dR.as<float>() : nullptr, gelu, tb, dC.as<float>(), (flags & 4) ? dCh.as<__half>() : nullptr, N, g_tune, nullptr);
            return true;
        };
        for (int i = 0; i < std::min(n_sets, 4); i++) if (!run(i)) return 4;
        HIP_CHECK(hipDeviceSynchronize());
        float ms = 0;
        timed(&ms, [&] { for (int i = 0; i < iters; i++) run(i % n_sets); return true; });
        if (us_per_launch) *us_per_launch = ms * 1e3f / (float)iters;
        return 0;
    });
}
// Micro-benchmark of the ViT / Q-Former attention (launch_attn_f32) on synthetic q|k|v rows: heads x hd wide, nq queries against nk keys, `iters` launches.
int minigpt4_amd_bench_attn_f32(int heads, int hd, int nq, int nk, int iters, float *us_per_launch) {
    if (heads < 1 || (hd != 88 && hd != 64) || nq < 1 || nk < 1 || nk > 320 || iters < 1) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int D = heads * hd, n = std::max(nq, nk);
        DevBuf dq((size_t)n * 3 * D * 4), dout((size_t)nq * D * 4), douth((size_t)nq * D * 2), dtab(65536 * 2);
        { std::vector<float> h((size_t)n * 3 * D); for (size_t i = 0; i < h.size(); i++) h[i] = (float)((int)(i * 2654435761u % 2001u) - 1000) / 1000.0f; HIP_CHECK(hipMemcpy(dq.p, h.data(), h.size() * 4, hipMemcpyHostToDevice)); }
        { std::vector<__half> e(65536); for (int i = 0; i < 65536; i++) e[(size_t)i] = __float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)i)))); HIP_CHECK(hipMemcpy(dtab.p, e.data(), 131072, hipMemcpyHostToDevice)); }
        Tables tb; tb.exp = dtab.as<__half>();
        { int nneg = 0; for (int c = 0x8000; c < 0xFC00; c++) { if (__half2float(__float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)c))))) == 0.0f) break; nneg++; } tb.exp_neg_n = (nneg + 2047) / 2048 * 2048; }
        const float scale = 1.0f / sqrtf((float)hd);
        auto run = [&]() { launch_attn_f32(dq.as<float>(), 3 * D, dq.as<float>() + D, dq.as<float>() + 2 * D, 3 * D, nq, nk, heads, hd, scale, 0.0f, tb, nullptr, douth.as<__half>(), D, g_tune, nullptr, 1); };
        for (int i = 0; i < 3; i++) run();
        HIP_CHECK(hipDeviceSynchronize());
        float ms = 0;
        timed(&ms, [&] { for (int i = 0; i < iters; i++) run(); return true; });
        if (us_per_launch) *us_per_launch = ms * 1e3f / (float)iters;
        return 0;
    });
}
// the same with `batch` images per launch, computed exponentials (what the engine's fast mode runs) and a forced number of query tiles per workgroup (0 = the launcher's choice)
int minigpt4_amd_bench_attn_f32_b(int heads, int hd, int nq, int nk, int batch, int qt, int iters, float *us_per_launch) {
    if (heads < 1 || (hd != 88 && hd != 64) || nq < 1 || nk < 1 || nk > 320 || iters < 1 || batch < 1 || batch > 16 || nq != nk) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int D = heads * hd;
        DevBuf dq((size_t)batch * nq * 3 * D * 4), douth((size_t)batch * nq * D * 2);
        { std::vector<float> h((size_t)batch * nq * 3 * D); for (size_t i = 0; i < h.size(); i++) h[i] = (float)((int)(i * 2654435761u % 2001u) - 1000) / 1000.0f; HIP_CHECK(hipMemcpy(dq.p, h.data(), h.size() * 4, hipMemcpyHostToDevice)); }
        Tables tb;                                                          // exp == null: computed exponentials
        const float scale = 1.0f / sqrtf((float)hd);
        LaunchTuning tune = hook_tuning(); tune.attn_vit_qt = qt; tune = tune.normalised();
        // MG4_ATTN_HEAD_MAJOR=1 (experiment): q | k | v as [3][head][batch x rows][hd] instead of [rows][3 x heads x hd]
        const bool hm = getenv("MG4_ATTN_HEAD_MAJOR") && atoi(getenv("MG4_ATTN_HEAD_MAJOR"));
        const int R = batch * nq;
        auto run = [&]() {
            if (hm) launch_attn_f32(dq.as<float>(), hd, dq.as<float>() + (size_t)D * R, dq.as<float>() + (size_t)2 * D * R, hd, nq, nk, heads, hd, scale, 0.0f, tb, nullptr, douth.as<__half>(), D, tune, nullptr, batch, R * hd, R * hd);
            else launch_attn_f32(dq.as<float>(), 3 * D, dq.as<float>() + D, dq.as<float>() + 2 * D, 3 * D, nq, nk, heads, hd, scale, 0.0f, tb, nullptr, douth.as<__half>(), D, tune, nullptr, batch); };
        for (int i = 0; i < 3; i++) run();
        HIP_CHECK(hipDeviceSynchronize());
        float ms = 0;
        timed(&ms, [&] { for (int i = 0; i < iters; i++) run(); return true; });
        if (us_per_launch) *us_per_launch = ms * 1e3f / (float)iters;
        return 0;
    });
}
void minigpt4_amd_test_set_attn_qt(int qt) { g_tune.attn_vit_qt = qt; g_tune = g_tune.normalised(); }
// The F16 feed-forward pair launch (launch_gemm_f16_silu_pair): x [N][n_in] fp32 (rounded to fp16 as the engine's row preparation does), w = w1 then w3, each [n_out][n_in]
// fp16; out_h [N][n_out] = fp16(silu_table(w1 x) * (w3 x)) as uint16 bit patterns, out_f (optional) the fp32 product before the rounding
static int test_f16_silu_pair_impl(const float *x, const void *w_f16, int64_t N, int64_t n_in, int64_t n_out, const unsigned short *table, unsigned short *out_h, float *out_f);
int minigpt4_amd_test_f16_silu_pair(const float *x, const void *w_f16, int64_t N, int64_t n_in, int64_t n_out, unsigned short *out_h, float *out_f) { return test_f16_silu_pair_impl(x, w_f16, N, n_in, n_out, host_silu_table().data(), out_h, out_f); }
// silu_table: the table the epilogue gathers from, or NULL: Tables::silu stays null -- the computed arm the engine's fast mode passes to this launch
int minigpt4_amd_test_f16_silu_pair_ex(const float *x, const void *w_f16, int64_t N, int64_t n_in, int64_t n_out, const unsigned short *silu_table, unsigned short *out_h, float *out_f) { return test_f16_silu_pair_impl(x, w_f16, N, n_in, n_out, silu_table, out_h, out_f); }
static int test_f16_silu_pair_impl(const float *x, const void *w_f16, int64_t N, int64_t n_in, int64_t n_out, const unsigned short *table, unsigned short *out_h, float *out_f) {
    if (!x || !w_f16 || !out_h || N <= 0 || n_in <= 0 || n_out <= 0) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t nx = (size_t)(N * n_in), nw = (size_t)(n_in * n_out), no = (size_t)(N * n_out);
        DevBuf dx(nx * 4), dxh(nx * 2), dw(nw * 2 * 2), dh(no * 2), df(no * 4), dtab(65536 * 2);
        HIP_CHECK(hipMemcpy(dx.p, x, nx * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dw.p, w_f16, nw * 4, hipMemcpyHostToDevice));
        Tables tb;
        if (table) { HIP_CHECK(hipMemcpy(dtab.p, table, 131072, hipMemcpyHostToDevice)); tb.silu = dtab.as<__half>(); }
        launch_f32_to_f16(dx.as<float>(), dxh.as<__half>(), nx, nullptr);
        hipDeviceProp_t prop; HIP_CHECK(hipGetDeviceProperties(&prop, 0));
        if (!launch_gemm_f16_silu_pair(dxh.as<__half>(), (int)n_in, dw.as<__half>(), dw.as<__half>() + nw, (int)N, (int)n_out, (int)n_in, tb, df.as<float>(), dh.as<__half>(), (int)n_out,
                                       g_tune, nullptr)) return 4;
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out_h, dh.p, no * 2, hipMemcpyDeviceToHost));
        if (out_f) HIP_CHECK(hipMemcpy(out_f, df.p, no * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// exp / SiLU / GELU (activations.hpp) over all 65 536 fp16 bit patterns: table != null gathers from it (uploaded), table == null computes -- the arm fast mode ships
int minigpt4_amd_test_activation(int which, const unsigned short *table, unsigned short *out) {
    if (which < 0 || which > 2 || !out) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        DevBuf dtab(65536 * 2), dout(65536 * 2);
        if (table) HIP_CHECK(hipMemcpy(dtab.p, table, 131072, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0xFF, 131072));
        hipLaunchKernelGGL(k_test_activation, dim3(256), dim3(256), 0, nullptr, which, table ? dtab.as<__half>() : nullptr, dout.as<unsigned short>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, dout.p, 131072, hipMemcpyDeviceToHost));
        return 0;
    });
}
// The ViT / Q-Former attention (launch_attn_f32 -> k_attn_vit) on host rows q [batch * nq][heads * hd], k / v [batch * nk][heads * hd] (an image's rows back to back).
// head_major: the rows are re-laid [head][batch * rows][hd] on the way to the device and the launch gets the head strides, as the ViT's qkv projection stores them; qt: query tiles
// per workgroup (0 = the launcher's choice; back at 0 afterwards); exp_table: ggml's fp16 exp table (gathered) or NULL (computed exponentials).  out / out_h: [batch * nq][heads * hd] fp32 / fp16 bits.
int minigpt4_amd_test_attn_f32(const float *q, const float *k, const float *v, int heads, int hd, int nq, int nk, int batch, float q_prescale, float score_div, int head_major, int qt,
                               const unsigned short *exp_table, float *out, unsigned short *out_h) {
    if (!q || !k || !v || !out || heads < 1 || (hd != 88 && hd != 64) || nq < 1 || nk < 1 || nk > 320 || batch < 1 || batch > 16 || qt < 0) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int D = heads * hd, Rq = batch * nq, Rk = batch * nk;
        const size_t nQ = (size_t)Rq * D, nK = (size_t)Rk * D;
        auto lay = [&](const float *src, int R) {   // [R][heads][hd] -> [heads][R][hd]
            std::vector<float> o((size_t)R * D);
            if (!head_major) { std::memcpy(o.data(), src, o.size() * 4); return o; }
            for (int r = 0; r < R; r++) for (int h = 0; h < heads; h++) std::memcpy(&o[((size_t)h * R + r) * hd], src + (size_t)r * D + (size_t)h * hd, (size_t)hd * 4);
            return o;
        };
        DevBuf dq(nQ * 4), dk(nK * 4), dv(nK * 4), dout(nQ * 4), douth(nQ * 2), dtab(65536 * 2);
        { const std::vector<float> hq = lay(q, Rq), hk = lay(k, Rk), hv = lay(v, Rk);
          HIP_CHECK(hipMemcpy(dq.p, hq.data(), nQ * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dk.p, hk.data(), nK * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, hv.data(), nK * 4, hipMemcpyHostToDevice)); }
        HIP_CHECK(hipMemset(dout.p, 0xFF, nQ * 4)); HIP_CHECK(hipMemset(douth.p, 0xFF, nQ * 2));
        Tables tb;
        if (exp_table) {   // as Engine::init sets the table up: the LDS part covers arguments -0 .. the last one whose entry is not zero, in whole 2048-entry pieces
            HIP_CHECK(hipMemcpy(dtab.p, exp_table, 131072, hipMemcpyHostToDevice)); tb.exp = dtab.as<__half>();
            int nneg = 0; for (int c = 0x8000; c < 0xFC00; c++) { if ((exp_table[c] & 0x7FFF) == 0) break; nneg++; }
            tb.exp_neg_n = (nneg + 2047) / 2048 * 2048;
        }
        LaunchTuning tune = hook_tuning(); tune.attn_vit_qt = qt; tune = tune.normalised();
        if (head_major) launch_attn_f32(dq.as<float>(), hd, dk.as<float>(), dv.as<float>(), hd, nq, nk, heads, hd, q_prescale, score_div, tb, dout.as<float>(), douth.as<__half>(), D, tune, nullptr, batch, Rq * hd, Rk * hd);
        else launch_attn_f32(dq.as<float>(), D, dk.as<float>(), dv.as<float>(), D, nq, nk, heads, hd, q_prescale, score_div, tb, dout.as<float>(), douth.as<__half>(), D, tune, nullptr, batch);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, dout.p, nQ * 4, hipMemcpyDeviceToHost));
        if (out_h) HIP_CHECK(hipMemcpy(out_h, douth.p, nQ * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}
// The context shift's kernel (launch_kv_shift) on host caches [n_layer][n_ctx][n_embd] fp16, with the RoPE table the engine builds (rope_tables)
int minigpt4_amd_test_kv_shift(int n_layer, int n_ctx, int n_embd, int n_head, int n_rows, int n_keep, int n_discard, uint16_t *k, uint16_t *v, float *ms) {
    if (!k || !v || n_layer < 1 || n_ctx < 1 || n_head < 1 || n_embd % n_head || (n_embd / n_head) % 8 || n_rows < 0 || n_rows > n_ctx || n_keep < 0 || n_discard < 0 ||
        n_keep + n_discard > n_rows) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int hd = n_embd / n_head;
        const size_t n = (size_t)n_layer * n_ctx * n_embd;
        std::vector<float> c, s;
        rope_tables(n_ctx, hd, c, s);
        DevBuf dk(n * 2), dv(n * 2), dc(c.size() * 4), ds(s.size() * 4);
        HIP_CHECK(hipMemcpy(dk.p, k, n * 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, v, n * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dc.p, c.data(), c.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(ds.p, s.data(), s.size() * 4, hipMemcpyHostToDevice));
        timed(ms, [&] { launch_kv_shift(dk.as<__half>(), dv.as<__half>(), n_layer, n_ctx, n_embd, hd, n_keep, n_discard, n_rows, dc.as<float>(), ds.as<float>(), nullptr); return true; });
        HIP_CHECK(hipMemcpy(k, dk.p, n * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(v, dv.p, n * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}
// The prefix copy's kernel (launch_kv_copy) on host caches [n_slot][n_layer][rows][n_embd] fp16: slot src (or a compact copy of its first src_rows rows) -> the slots dst.
// k == v == NULL: timing only, on device buffers of that shape that never cross the host (the engine's real strides, n_ctx = 2048 rows per layer, are gigabytes per tensor)
int minigpt4_amd_test_kv_copy(int n_slot, int n_layer, int rows, int n_embd, int src, const int32_t *dst, int n_dst, int n_rows, int src_rows, uint16_t *k, uint16_t *v, float *ms) {
    if (!k != !v || !dst || n_slot < 1 || n_layer < 1 || rows < 1 || n_embd < 1 || src < 0 || src >= n_slot || n_dst < 1 || n_dst > KV_COPY_MAX_DST || src_rows < 0 || src_rows > rows) return 1;
    for (int i = 0; i < n_dst; i++) if (dst[i] < 0 || dst[i] >= n_slot || dst[i] == src) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t E = (size_t)n_embd, slot_n = (size_t)n_layer * rows * E, n = (size_t)n_slot * slot_n;
        DevBuf dk(n * 2), dv(n * 2), ck(src_rows ? (size_t)n_layer * src_rows * E * 2 : 2), cv(src_rows ? (size_t)n_layer * src_rows * E * 2 : 2);
        if (k) { HIP_CHECK(hipMemcpy(dk.p, k, n * 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, v, n * 2, hipMemcpyHostToDevice)); }
        else { HIP_CHECK(hipMemset(dk.p, 0x11, n * 2)); HIP_CHECK(hipMemset(dv.p, 0x22, n * 2)); }   // every page touched before the timed launch
        const __half *sk = dk.as<__half>() + (size_t)src * slot_n, *sv = dv.as<__half>() + (size_t)src * slot_n;
        if (src_rows) {   // [layer][rows][E] -> [layer][src_rows][E]
            HIP_CHECK(hipMemcpy2D(ck.p, (size_t)src_rows * E * 2, sk, (size_t)rows * E * 2, (size_t)src_rows * E * 2, (size_t)n_layer, hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy2D(cv.p, (size_t)src_rows * E * 2, sv, (size_t)rows * E * 2, (size_t)src_rows * E * 2, (size_t)n_layer, hipMemcpyDeviceToDevice));
            sk = ck.as<__half>(); sv = cv.as<__half>();
        }
        KvCopyDst d{};
        for (int i = 0; i < n_dst; i++) { d.k[i] = dk.as<__half>() + (size_t)dst[i] * slot_n; d.v[i] = dv.as<__half>() + (size_t)dst[i] * slot_n; }
        timed(ms, [&] { launch_kv_copy(sk, sv, src_rows ? src_rows : rows, d, n_dst, rows, n_layer, n_embd, n_rows, nullptr); return true; });
        if (k) { HIP_CHECK(hipMemcpy(k, dk.p, n * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(v, dv.p, n * 2, hipMemcpyDeviceToHost)); }
        return 0;
    });
}
// device_checksum (k_checksum: the sum of the 32-bit words mod 2^64) over a caller-given device-accessible range -- tools/state_swap.py's baseline runs it over the pinned
// block its runtime copies filled.  ms: hipEvent time around the call (the launch, and the 8-byte allocation, memset and copy back that device_checksum makes)
int minigpt4_amd_test_checksum(const void *device_ptr, size_t bytes, uint64_t *sum_out, float *ms) {
    if (!device_ptr || !sum_out || (uintptr_t)device_ptr % 4) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        timed(ms, [&] { *sum_out = device_checksum(device_ptr, bytes, nullptr); return true; });
        return 0;
    });
}
// The snapshot kernels alone (launch_kv_pack / launch_kv_unpack) on host caches [n_layer][n_ctx][n_embd] fp16 of ONE conversation and a host block [2][n_layer][n][n_embd].
// The row range is NOT checked here: the launcher's refusal is what the tests look at (rc 3).  k == v == block == NULL: timing only, on device buffers of that shape that
// never cross the host (the engine's real strides are gigabytes per tensor)
int minigpt4_amd_test_kv_pack(int n_layer, int n_ctx, int n_embd, int r0, int n, const uint16_t *k, const uint16_t *v, uint16_t *block_out, uint64_t *sum_out, float *ms) {
    if (!k != !v || !k != !block_out || !sum_out || n_layer < 1 || n_ctx < 1 || n_embd < 1 || n < 0 || n > n_ctx) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t cache = (size_t)n_layer * n_ctx * n_embd * 2, blk = (size_t)2 * n_layer * n * n_embd * 2;
        DevBuf dk(cache), dv(cache), db(blk), ds(8);
        if (k) { HIP_CHECK(hipMemcpy(dk.p, k, cache, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, v, cache, hipMemcpyHostToDevice)); }
        else { HIP_CHECK(hipMemset(dk.p, 0x11, cache)); HIP_CHECK(hipMemset(dv.p, 0x22, cache)); }   // every page touched before the timed launch
        HIP_CHECK(hipMemset(db.p, 0, blk ? blk : 1)); HIP_CHECK(hipMemset(ds.p, 0xFF, 8));   // the launcher zeroes the word
        timed(ms, [&] { launch_kv_pack(dk.as<__half>(), dv.as<__half>(), n_ctx, n_layer, n_embd, r0, n, db.as<__half>(), ds.as<unsigned long long>(), nullptr); return true; });
        if (blk && block_out) HIP_CHECK(hipMemcpy(block_out, db.p, blk, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(sum_out, ds.p, 8, hipMemcpyDeviceToHost));
        return 0;
    });
}
int minigpt4_amd_test_kv_unpack(int n_layer, int n_ctx, int n_embd, int r0, int n, const uint16_t *block, uint16_t *k, uint16_t *v, uint64_t *sum_out, float *ms) {
    if (!k != !v || !k != !block || !sum_out || n_layer < 1 || n_ctx < 1 || n_embd < 1 || n < 0 || n > n_ctx) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t cache = (size_t)n_layer * n_ctx * n_embd * 2, blk = (size_t)2 * n_layer * n * n_embd * 2;
        DevBuf dk(cache), dv(cache), db(blk), ds(8);
        if (k) { HIP_CHECK(hipMemcpy(dk.p, k, cache, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, v, cache, hipMemcpyHostToDevice)); }
        else { HIP_CHECK(hipMemset(dk.p, 0x11, cache)); HIP_CHECK(hipMemset(dv.p, 0x22, cache)); }
        if (blk && block) HIP_CHECK(hipMemcpy(db.p, block, blk, hipMemcpyHostToDevice));
        else if (blk) HIP_CHECK(hipMemset(db.p, 0x33, blk));
        HIP_CHECK(hipMemset(ds.p, 0xFF, 8));
        timed(ms, [&] { launch_kv_unpack(db.as<__half>(), dk.as<__half>(), dv.as<__half>(), n_ctx, n_layer, n_embd, r0, n, ds.as<unsigned long long>(), nullptr); return true; });
        if (k) { HIP_CHECK(hipMemcpy(k, dk.p, cache, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(v, dv.p, cache, hipMemcpyDeviceToHost)); }
        HIP_CHECK(hipMemcpy(sum_out, ds.p, 8, hipMemcpyDeviceToHost));
        return 0;
    });
}
// The scoring kernel (launch_logprob_rows) on host logits [rows][ld]: one launch, hipEvent-timed.  Every target is checked here: it indexes a row on the device.
int minigpt4_amd_test_logprob_rows(const float *logits, int rows, int n_vocab, int ld, const int32_t *targets, float *logprob_out, int32_t *greedy_out, float *greedy_logprob_out,
                                   float *ms_out) {
    if (!logits || !targets || !logprob_out || !greedy_out || !greedy_logprob_out || rows < 1 || n_vocab < 1 || ld < n_vocab) return 1;
    for (int r = 0; r < rows; r++) if (targets[r] < -1 || targets[r] >= n_vocab) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)rows * ld, R = (size_t)rows;
        DevBuf dl(n * 4), dt(R * 4), dp(R * 4), dg(R * 4), dq(R * 4);
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dt.p, targets, R * 4, hipMemcpyHostToDevice));
        timed(ms_out, [&] { launch_logprob_rows(dl.as<float>(), ld, n_vocab, rows, dt.as<int>(), dp.as<float>(), dg.as<int>(), dq.as<float>(), nullptr); return true; });
        HIP_CHECK(hipMemcpy(logprob_out, dp.p, R * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(greedy_out, dg.p, R * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(greedy_logprob_out, dq.p, R * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// The top-N kernel (launch_topn_rows) on host logits [buf_rows][ld]: one launch, hipEvent-timed.  Everything that indexes device memory is checked here.
int minigpt4_amd_test_topn_rows(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *row_index, int rows, int top_n, const int32_t *targets, int32_t *ids_out,
                                float *logprobs_out, int32_t *rank_out, float *target_logprob_out, float *ms_out) {
    if (!logits || !targets || !ids_out || !logprobs_out || !rank_out || !target_logprob_out || rows < 1 || buf_rows < 1 || n_vocab < 1 || ld < n_vocab) return 1;
    if (top_n < 1 || top_n > TOPN_MAX || top_n > n_vocab) return 1;
    if (!row_index && rows > buf_rows) return 1;
    for (int r = 0; r < rows; r++) {
        if (targets[r] < -1 || targets[r] >= n_vocab) return 1;
        if (row_index && (row_index[r] < 0 || row_index[r] >= buf_rows)) return 1;
    }
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)buf_rows * ld, R = (size_t)rows, RN = R * (size_t)top_n;
        DevBuf dl(n * 4), dt(R * 4), dx(R * 4), di(RN * 4), dp(RN * 4), dr(R * 4), dq(R * 4);
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dt.p, targets, R * 4, hipMemcpyHostToDevice));
        if (row_index) HIP_CHECK(hipMemcpy(dx.p, row_index, R * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(di.p, 0xFF, RN * 4)); HIP_CHECK(hipMemset(dp.p, 0xFF, RN * 4));   // an entry the kernel leaves out shows as id -1 / NaN
        if (!timed(ms_out, [&] { return launch_topn_rows(dl.as<float>(), ld, n_vocab, rows, row_index ? dx.as<int>() : nullptr, top_n, dt.as<int>(), di.as<int>(), dp.as<float>(), dr.as<int>(), dq.as<float>(), nullptr); })) return 3;
        HIP_CHECK(hipMemcpy(ids_out, di.p, RN * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(logprobs_out, dp.p, RN * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(rank_out, dr.p, R * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(target_logprob_out, dq.p, R * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// ---- beam search (beam.hpp, beam_host.hpp) ----
static bool beam_hook_args_ok(int W, int n_steps, const int32_t *ids, const float *lp) { return W >= 2 && W <= BEAM_MAX && n_steps >= 1 && ids && lp; }
// The rule on the CPU: n_steps steps whose candidates are GIVEN -- ids / logprobs [n_steps][W][2 W], row (t, i) = what beam i lists in step t, in k_topn_rows' order -- through
// beam_select_host and the engine's book-keeping (BeamBook) at source position `position`.  scores0 / live0: the first step's beam scores and live mask (NULL: the search's own
// first step, only beam 0 live).  steps_out (may be NULL): [steps run][44] words, every step's BeamStep.
int minigpt4_amd_test_beam_select_host(int n_beams, int n_steps, const int32_t *ids, const float *logprobs, const float *scores0, uint32_t live0, int eos, int position,
                                       float length_penalty, int n_best, int32_t *steps_out, int32_t *tokens_out, int32_t *lengths_out, float *scores_out, int32_t *n_out,
                                       int32_t *stats) {
    const int W = n_beams, C = 2 * W;
    if (!beam_hook_args_ok(W, n_steps, ids, logprobs) || n_best < 1 || n_best > W || !tokens_out || !lengths_out || !scores_out || !n_out || !stats || position < 0) return 1;
    if (scores0 && !(live0 & ((1u << W) - 1u))) return 1;
    if (!std::isfinite(length_penalty)) return 1;
    BeamBook book(W, position, length_penalty);
    float s[BEAM_MAX];
    for (int i = 0; i < BEAM_MAX; i++) s[i] = scores0 && i < W ? scores0[i] : (i == 0 ? 0.0f : -INFINITY);
    for (int t = 0; t < n_steps && !book.full; t++) {
        BeamStep r;
        beam_select_host(W, C, s, t == 0 ? (scores0 ? live0 : 1u) : (1u << W) - 1u, ids + (size_t)t * W * C, logprobs + (size_t)t * W * C, eos, r);
        if (steps_out) memcpy(steps_out + (size_t)t * (sizeof(BeamStep) / 4), &r, sizeof(BeamStep));
        if (r.n_live != W) return 1;                                          // fewer than W tokens other than EOS among the live candidates: not a step of the search
        for (int i = 0; i < W; i++) s[i] = r.score[i];
        book.step(r);
    }
    book.finish();
    *n_out = book.write(n_best, n_steps + 1, tokens_out, lengths_out, scores_out);
    for (int i = 0; i < 4; i++) stats[i] = book.stats[i];
    return 0;
}
// k_beam_select, one launch: ids / logprobs [W][2 W], scores [W] (updated in place like the device copy), the result block and the row tokens it wrote
int minigpt4_amd_test_beam_select(int n_beams, const int32_t *ids, const float *logprobs, float *scores, uint32_t live, int eos, int n_vocab, int32_t *step_out, int32_t *row_tok_out) {
    const int W = n_beams, C = 2 * W;
    if (!beam_hook_args_ok(W, 1, ids, logprobs) || !scores || !step_out || !row_tok_out || n_vocab < 1 || !(live & ((1u << W) - 1u))) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)W * C;
        DevBuf di(n * 4), dl(n * 4), ds(BEAM_MAX * 4), dr(sizeof(BeamStep)), dt(BEAM_MAX * 4);
        HIP_CHECK(hipMemcpy(di.p, ids, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dl.p, logprobs, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(ds.p, scores, (size_t)W * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dr.p, 0xFF, sizeof(BeamStep))); HIP_CHECK(hipMemset(dt.p, 0xFF, BEAM_MAX * 4));
        if (!launch_beam_select(di.as<int>(), dl.as<float>(), ds.as<float>(), live, W, C, eos, n_vocab, static_cast<BeamStep *>(dr.p), dt.as<int>(), nullptr)) return 3;
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(step_out, dr.p, sizeof(BeamStep), hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(row_tok_out, dt.p, (size_t)W * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(scores, ds.p, (size_t)W * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// k_kv_permute on host caches k / v = [n_slot][n_layer][n_ctx][n_embd] fp16 (changed in place): listed slot i receives rows [r0, r1) of listed slot parent[i].
// k == v == NULL: timing only, on device buffers of that shape
int minigpt4_amd_test_kv_permute(int n_slot, int n_layer, int n_ctx, int n_embd, const int32_t *slots, int n, const int32_t *parent, int r0, int r1, uint16_t *k, uint16_t *v,
                                 float *ms) {
    if (!k != !v || !slots || !parent || n_slot < 1 || n_layer < 1 || n_ctx < 1 || n_embd < 1 || n < 2 || n > KV_PERMUTE_MAX || n > n_slot) return 1;
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= n_slot || parent[i] < 0 || parent[i] >= n) return 1;
        for (int j = 0; j < i; j++) if (slots[j] == slots[i]) return 1;
    }
    if (r0 < 0 || r1 < r0 || r1 > n_ctx) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t slot_n = (size_t)n_layer * n_ctx * n_embd, total = (size_t)n_slot * slot_n;
        DevBuf dk(total * 2), dv(total * 2), dp(KV_PERMUTE_MAX * 4);
        if (k) { HIP_CHECK(hipMemcpy(dk.p, k, total * 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, v, total * 2, hipMemcpyHostToDevice)); }
        else { HIP_CHECK(hipMemset(dk.p, 0x11, total * 2)); HIP_CHECK(hipMemset(dv.p, 0x22, total * 2)); }
        HIP_CHECK(hipMemcpy(dp.p, parent, (size_t)n * 4, hipMemcpyHostToDevice));
        KvPermuteSlots ps{};
        for (int i = 0; i < n; i++) ps.s[i] = slots[i];
        timed(ms, [&] { launch_kv_permute(dk.as<__half>(), dv.as<__half>(), slot_n, n_slot, ps, n, dp.as<int>(), n_layer, n_ctx, n_embd, r0, r1, nullptr); return true; });
        if (k) { HIP_CHECK(hipMemcpy(k, dk.p, total * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(v, dv.p, total * 2, hipMemcpyDeviceToHost)); }
        return 0;
    });
}
// ---- penalties and logit bias (penalty.hpp) ----
int minigpt4_amd_test_penalise_host(float *row, int n_vocab, const int32_t *history, int n_history, int n_ctx, int32_t repeat_last_n, float repeat_penalty, float alpha_presence,
                                    float alpha_frequency, int penalize_nl, const int32_t *bias_ids, const float *bias, int n_bias, int32_t *table_out, int table_cap, int32_t *flags_out) {
    if (!row || n_vocab < 1 || n_history < 0 || (n_history > 0 && !history) || n_bias < 0 || n_bias > PEN_BIAS_MAX || (n_bias > 0 && (!bias_ids || !bias))) return -1;
    for (int i = 0; i < n_bias; i++) {
        if (bias_ids[i] < 0 || bias_ids[i] >= n_vocab) return -1;
        for (int j = 0; j < i; j++) if (bias_ids[j] == bias_ids[i]) return -1;
    }
    try {
        const PenParams p{repeat_last_n, repeat_penalty, alpha_presence, alpha_frequency, penalize_nl};
        std::vector<PenEntry> tab;
        const int flags = pen_build_table(history, (size_t)n_history, p, n_ctx, n_vocab, bias_ids, bias, n_bias, tab);
        pen_apply_row(row, n_vocab, tab, flags, p);
        static_assert(sizeof(PenEntry) == 16, "the hooks hand tables out as 4 words per entry");
        if (table_out) memcpy(table_out, tab.data(), std::min(tab.size(), (size_t)std::max(table_cap, 0)) * sizeof(PenEntry));
        if (flags_out) *flags_out = flags;
        return (int)tab.size();
    } catch (...) { return -1; }
}
int minigpt4_amd_test_pen_pick(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *rows, int n_rows, const int32_t *table, int n_table, int32_t *picked_out,
                               float *adjusted_out, float *ms_out) {
    static_assert(sizeof(PenRow) == 32 && sizeof(PenEntry) == 16, "the hook's word layout");
    if (!logits || !rows || !picked_out || buf_rows < 1 || n_vocab < 1 || ld < n_vocab || n_rows < 1 || n_table < 0 || (n_table > 0 && !table)) return 1;
    if (!pen_rows_ok(rows, n_rows, table, n_table, buf_rows, n_vocab)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)buf_rows * ld, R = (size_t)n_rows, T = (size_t)std::max(n_table, 1);
        DevBuf dl(n * 4), dr(R * sizeof(PenRow)), dt(T * sizeof(PenEntry)), dp(R * 4), da(T * 4);
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dr.p, rows, R * sizeof(PenRow), hipMemcpyHostToDevice));
        if (n_table > 0) HIP_CHECK(hipMemcpy(dt.p, table, (size_t)n_table * sizeof(PenEntry), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dp.p, 0xFF, R * 4)); HIP_CHECK(hipMemset(da.p, 0xFF, T * 4));   // what the kernel leaves out shows as id -1 / NaN
        if (!timed(ms_out, [&] { return launch_pen_pick(dl.as<float>(), ld, n_vocab, n_rows, dr.as<PenRow>(), dt.as<PenEntry>(), dp.as<int>(), da.as<float>(), nullptr); })) return 3;
        HIP_CHECK(hipMemcpy(picked_out, dp.p, R * 4, hipMemcpyDeviceToHost));
        if (adjusted_out && n_table > 0) HIP_CHECK(hipMemcpy(adjusted_out, da.p, (size_t)n_table * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// ---- constrained decoding (constraint.hpp, launch_constrain_index, launch_constrain_pick) ----
int minigpt4_amd_test_constraint_compile(const char *pattern, int n_bytes, uint16_t *trans_out, uint32_t *accept_out, int cap_states, int32_t *n_states_out, char *err, size_t err_cap) {
    if (!pattern || !n_states_out) return -1;
    if (err && err_cap) err[0] = 0;
    try {
        ConstraintDfa dfa; std::string why;
        if (!constraint_compile(reinterpret_cast<const unsigned char *>(pattern), n_bytes < 0 ? strlen(pattern) : (size_t)n_bytes, dfa, why)) {
            if (err && err_cap) { strncpy(err, why.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
            return 1;
        }
        *n_states_out = dfa.n_states;
        if (trans_out && cap_states >= dfa.n_states) memcpy(trans_out, dfa.trans.data(), dfa.trans.size() * 2);
        if (accept_out) { memset(accept_out, 0, 32 * 4); memcpy(accept_out, dfa.accept.data(), dfa.accept.size() * 4); }
        return 0;
    } catch (...) { return -1; }
}
int minigpt4_amd_test_constrain_index(const uint8_t *vocab, const int32_t *off, int n_vocab, const uint16_t *trans, const uint32_t *accept, int n_states, uint32_t *index_out,
                                      float *ms_out) {
    if (!vocab || !off || !trans || !accept || !index_out || n_vocab < 1 || n_states < 2 || n_states > CONSTRAINT_MAX_STATES || off[0] != 0) return 1;
    for (int i = 0; i < n_vocab; i++) if (off[i + 1] < off[i]) return 1;                       // everything that indexes device memory
    for (size_t i = 0; i < (size_t)n_states * 256; i++) if (trans[i] >= n_states) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t nb = (size_t)off[n_vocab], S = (size_t)n_states, W = (size_t)constraint_words(n_vocab), A = (S + 31) / 32;
        DevBuf dv(std::max<size_t>(nb, 1)), doff(((size_t)n_vocab + 1) * 4), dt(S * 512), da(A * 4), di(S * W * 4);
        if (nb) HIP_CHECK(hipMemcpy(dv.p, vocab, nb, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(doff.p, off, ((size_t)n_vocab + 1) * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dt.p, trans, S * 512, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(da.p, accept, A * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(di.p, 0xA5, S * W * 4));                                           // a word the kernel leaves out shows
        if (!timed(ms_out, [&] { return launch_constrain_index(dv.as<unsigned char>(), doff.as<int>(), n_vocab, dt.as<uint16_t>(), da.as<unsigned>(), n_states, di.as<unsigned>(), nullptr); })) return 3;
        HIP_CHECK(hipMemcpy(index_out, di.p, S * W * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
int minigpt4_amd_test_constrain_pick(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *rows, int n_rows, const int32_t *table, int n_table,
                                     const uint32_t *bitmaps, int n_bitmaps, const int32_t *bitmap_of_row, int32_t *out, float *ms_out) {
    static_assert(sizeof(PenRow) == 32 && sizeof(PenEntry) == 16 && sizeof(ConRow) == 48, "the hook's word layout");
    if (!logits || !rows || !out || !bitmaps || !bitmap_of_row || buf_rows < 1 || n_vocab < 1 || ld < n_vocab || n_rows < 1 || n_bitmaps < 1 || n_table < 0 || (n_table > 0 && !table)) return 1;
    if (!pen_rows_ok(rows, n_rows, table, n_table, buf_rows, n_vocab)) return 1;
    for (int r = 0; r < n_rows; r++) if (bitmap_of_row[r] < 0 || bitmap_of_row[r] >= n_bitmaps) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)buf_rows * ld, R = (size_t)n_rows, T = (size_t)std::max(n_table, 1), W = (size_t)constraint_words(n_vocab);
        DevBuf dl(n * 4), dr(R * sizeof(ConRow)), dt(T * sizeof(PenEntry)), dp(R * 4), db((size_t)n_bitmaps * W * 4);
        std::vector<ConRow> tab(R);
        for (size_t r = 0; r < R; r++) { memcpy(&tab[r].pen, rows + 8 * r, sizeof(PenRow)); tab[r].allowed = db.as<unsigned>() + (size_t)bitmap_of_row[r] * W; tab[r].pad = 0; }
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dr.p, tab.data(), R * sizeof(ConRow), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(db.p, bitmaps, (size_t)n_bitmaps * W * 4, hipMemcpyHostToDevice));
        if (n_table > 0) HIP_CHECK(hipMemcpy(dt.p, table, (size_t)n_table * sizeof(PenEntry), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dp.p, 0xFF, R * 4));                                                // what the kernel leaves out shows as id -1
        if (!timed(ms_out, [&] { return launch_constrain_pick(dl.as<float>(), ld, n_vocab, n_rows, dr.as<ConRow>(), dt.as<PenEntry>(), dp.as<int>(), nullptr); })) return 3;
        HIP_CHECK(hipMemcpy(out, dp.p, R * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// ---- guided decoding (launch_guide_rows) ----
// k_guide_rows, one launch, on host logits [buf_rows][ld]: pairs = [n][2] buffer rows (guided, guidance), scales[n], row_tok_index = [n][2] indices into a 64-entry row-token
// array (-1: not written) that starts as row_tok_io and is returned there.  mixed_out (may be NULL): [n][n_vocab].  Everything that indexes device memory is checked here.
int minigpt4_amd_test_guide_rows(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *pairs, const float *scales, const int32_t *row_tok_index, int n,
                                 float *mixed_out, int32_t *pick_out, float *pick_value_out, int32_t *row_tok_io, float *ms_out) {
    if (!logits || !pairs || !scales || !row_tok_index || !pick_out || !pick_value_out || !row_tok_io || buf_rows < 1 || n_vocab < 1 || ld < n_vocab || n < 1 || n > GUIDE_MAX) return 1;
    for (int i = 0; i < 2 * n; i++) if (pairs[i] < 0 || pairs[i] >= buf_rows || row_tok_index[i] < -1 || row_tok_index[i] >= 64) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        static_assert(sizeof(GuidePair) == 32, "the pair table is 8 words per pair");
        const size_t total = (size_t)buf_rows * ld, P = (size_t)n, PV = P * (size_t)n_vocab;
        std::vector<GuidePair> tab(P);
        for (int i = 0; i < n; i++) tab[(size_t)i] = GuidePair{pairs[2 * i], pairs[2 * i + 1], scales[i], row_tok_index[2 * i], row_tok_index[2 * i + 1], {0, 0, 0}};
        DevBuf dl(total * 4), dt(P * sizeof(GuidePair)), dm(PV * 4), dp(P * 4), dv(P * 4), dr(64 * 4);
        HIP_CHECK(hipMemcpy(dl.p, logits, total * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dt.p, tab.data(), P * sizeof(GuidePair), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dr.p, row_tok_io, 64 * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dm.p, 0xFF, PV * 4)); HIP_CHECK(hipMemset(dp.p, 0xFF, P * 4)); HIP_CHECK(hipMemset(dv.p, 0xFF, P * 4));   // what the kernel leaves out shows as NaN / id -1
        if (!timed(ms_out, [&] { return launch_guide_rows(dl.as<float>(), ld, n_vocab, n, dt.as<GuidePair>(), mixed_out ? dm.as<float>() : nullptr, dp.as<int>(), dv.as<float>(), dr.as<int>(), nullptr); })) return 3;
        if (mixed_out) HIP_CHECK(hipMemcpy(mixed_out, dm.p, PV * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(pick_out, dp.p, P * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(pick_value_out, dv.p, P * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(row_tok_io, dr.p, 64 * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// ---- device-side sampling (sampling.hpp, launch_sample_rows) ----
int minigpt4_amd_test_philox(const uint32_t *counter, const uint32_t *key, uint32_t *out) {
    if (!counter || !key || !out) return 1;
    philox4x32_10(counter, key, out);
    return 0;
}
int minigpt4_amd_test_sample_rule(const float *values, int n_cand, float temp, float top_p, uint32_t word, float *p_out, int32_t *kept_out) {
    if (!values || !p_out || !kept_out || n_cand < 1 || n_cand > SAMPLE_MAX || !(temp > 0.0f) || !std::isfinite(temp) || !(top_p > 0.0f)) return -1;
    int kept = 0;
    const int pick = sample_rule(values, n_cand, temp, top_p, word, p_out, &kept);
    *kept_out = kept;
    return pick;
}
// k_sample_rows, one launch, on host logits [buf_rows][ld].  Everything that indexes device memory is checked here.
int minigpt4_amd_test_sample_rows(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *rows, int n_rows, const int32_t *table, int n_table, const uint32_t *bitmaps,
                                  int n_bitmaps, const int32_t *bitmap_of_row, const float *temp_top_p, const int32_t *top_k, const uint64_t *seed_draws, const int32_t *tok_index,
                                  int32_t *row_tok_io, int32_t *out, float *ms_out) {
    static_assert(sizeof(PenRow) == 32 && sizeof(PenEntry) == 16 && sizeof(SampleRow) == 72 && sizeof(SampleOut) == (5 + 2 * SAMPLE_MAX) * 4, "the hook's word layout");
    if (!logits || !rows || !bitmap_of_row || !temp_top_p || !top_k || !seed_draws || !tok_index || !row_tok_io || !out || buf_rows < 1 || n_vocab < 1 || ld < n_vocab || n_rows < 1 ||
        n_table < 0 || (n_table > 0 && !table) || n_bitmaps < 0 || (n_bitmaps > 0 && !bitmaps)) return 1;
    if (!pen_rows_ok(rows, n_rows, table, n_table, buf_rows, n_vocab)) return 1;
    for (int r = 0; r < n_rows; r++) {   // the other indices, and the parameters the engine checks
        if (bitmap_of_row[r] < -1 || bitmap_of_row[r] >= n_bitmaps || tok_index[r] < -1 || tok_index[r] >= 64 || top_k[r] < 1 || top_k[r] > std::min(SAMPLE_MAX, n_vocab)) return 1;
        const float temp = temp_top_p[2 * (size_t)r], top_p = temp_top_p[2 * (size_t)r + 1];
        if (!std::isfinite(temp) || !(temp > 0.0f) || !(top_p > 0.0f) || !(top_p <= 1.0f)) return 1;
    }
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)buf_rows * ld, R = (size_t)n_rows, T = (size_t)std::max(n_table, 1), W = (size_t)constraint_words(n_vocab), NB = (size_t)std::max(n_bitmaps, 1);
        DevBuf dl(n * 4), dr(R * sizeof(SampleRow)), dt(T * sizeof(PenEntry)), dout(R * sizeof(SampleOut)), db(NB * W * 4), dtok(64 * 4);
        std::vector<SampleRow> tab(R);
        for (size_t r = 0; r < R; r++) {
            memcpy(&tab[r].pen, rows + 8 * r, sizeof(PenRow));
            tab[r].allowed = bitmap_of_row[r] < 0 ? nullptr : db.as<unsigned>() + (size_t)bitmap_of_row[r] * W;
            tab[r].temp = temp_top_p[2 * r]; tab[r].top_p = temp_top_p[2 * r + 1]; tab[r].top_k = top_k[r]; tab[r].tok_index = tok_index[r];
            tab[r].seed = seed_draws[2 * r]; tab[r].draws = seed_draws[2 * r + 1];
        }
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dr.p, tab.data(), R * sizeof(SampleRow), hipMemcpyHostToDevice));
        if (n_bitmaps > 0) HIP_CHECK(hipMemcpy(db.p, bitmaps, (size_t)n_bitmaps * W * 4, hipMemcpyHostToDevice));
        if (n_table > 0) HIP_CHECK(hipMemcpy(dt.p, table, (size_t)n_table * sizeof(PenEntry), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dtok.p, row_tok_io, 64 * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0xFF, R * sizeof(SampleOut)));                              // what the kernel leaves out shows as -1 / NaN
        if (!timed(ms_out, [&] { return launch_sample_rows(dl.as<float>(), ld, n_vocab, n_rows, dr.as<SampleRow>(), dt.as<PenEntry>(), dout.as<SampleOut>(), dtok.as<int>(), nullptr); })) return 3;
        HIP_CHECK(hipMemcpy(out, dout.p, R * sizeof(SampleOut), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(row_tok_io, dtok.p, 64 * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// ---- the extended rule (sampling.hpp: sample_chain; launch_sample_rows_ex) ----
// the ranges every caller of the chain checks (the engine's chain_params_ok states them with words)
static bool chain_ok(float tfs_z, float typical_p, float min_p, int mirostat, float tau, float eta) {
    return tfs_z > 0.0f && tfs_z <= 1.0f && typical_p > 0.0f && typical_p <= 1.0f && min_p >= 0.0f && min_p <= 1.0f && (mirostat == 0 || mirostat == 2) && std::isfinite(tau) &&
           tau > 0.0f && std::isfinite(eta) && eta >= 0.0f;
}
int minigpt4_amd_test_sample_chain(const float *values, int n_cand, float temp, float top_p, float tfs_z, float typical_p, float min_p, int mirostat, float tau, float eta, float mu,
                                   uint32_t word, float *p_out, int32_t *kept_out, uint64_t *mask_out, float *mu_out, float *observed_out) {
    if (!values || !p_out || !kept_out || !mask_out || !mu_out || !observed_out || n_cand < 1 || n_cand > SAMPLE_MAX || !(temp > 0.0f) || !std::isfinite(temp) || !(top_p > 0.0f) ||
        !chain_ok(tfs_z, typical_p, min_p, mirostat, tau, eta) || std::isinf(mu)) return -1;
    float sa[SAMPLE_MAX], sb[SAMPLE_MAX]; int L[SAMPLE_MAX], ord[SAMPLE_MAX];
    const ChainParams cp{tfs_z, typical_p, min_p, mirostat, tau, eta, mu, 0};
    ChainRes res{};
    sample_chain(values, n_cand, temp, top_p, cp, word, 0, 1, p_out, sa, sb, L, ord, &res);
    *kept_out = res.kept; *mask_out = (uint64_t)res.mask_lo | (uint64_t)res.mask_hi << 32; *mu_out = res.mu; *observed_out = res.observed;
    return res.pick;
}
// k_sample_rows_ex, one launch, on host logits [buf_rows][ld].  Everything that indexes device memory is checked here.
int minigpt4_amd_test_sample_rows_ex(const float *logits, int buf_rows, int n_vocab, int ld, const int32_t *rows, int n_rows, const int32_t *table, int n_table, const uint32_t *bitmaps,
                                     int n_bitmaps, const int32_t *bitmap_of_row, const float *temp_top_p, const int32_t *top_k, const uint64_t *seed_draws, const int32_t *tok_index,
                                     const float *chain, const int32_t *mirostat, int32_t *row_tok_io, int32_t *out, float *ms_out) {
    static_assert(sizeof(PenRow) == 32 && sizeof(PenEntry) == 16 && sizeof(SampleRowEx) == 104 && sizeof(SampleOutEx) == (9 + 2 * SAMPLE_MAX) * 4, "the hook's word layout");
    if (!logits || !rows || !bitmap_of_row || !temp_top_p || !top_k || !seed_draws || !tok_index || !chain || !mirostat || !row_tok_io || !out || buf_rows < 1 || n_vocab < 1 ||
        ld < n_vocab || n_rows < 1 || n_table < 0 || (n_table > 0 && !table) || n_bitmaps < 0 || (n_bitmaps > 0 && !bitmaps)) return 1;
    if (!pen_rows_ok(rows, n_rows, table, n_table, buf_rows, n_vocab)) return 1;
    for (int r = 0; r < n_rows; r++) {   // the other indices, and the parameters the engine checks
        if (bitmap_of_row[r] < -1 || bitmap_of_row[r] >= n_bitmaps || tok_index[r] < -1 || tok_index[r] >= 64 || top_k[r] < 1 || top_k[r] > std::min(SAMPLE_MAX, n_vocab)) return 1;
        const float temp = temp_top_p[2 * (size_t)r], top_p = temp_top_p[2 * (size_t)r + 1], *c = chain + 6 * (size_t)r;
        if (!std::isfinite(temp) || !(temp > 0.0f) || !(top_p > 0.0f) || !(top_p <= 1.0f) || !chain_ok(c[0], c[1], c[2], mirostat[r], c[3], c[4]) || std::isinf(c[5])) return 1;
    }
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)buf_rows * ld, R = (size_t)n_rows, T = (size_t)std::max(n_table, 1), W = (size_t)constraint_words(n_vocab), NB = (size_t)std::max(n_bitmaps, 1);
        DevBuf dl(n * 4), dr(R * sizeof(SampleRowEx)), dt(T * sizeof(PenEntry)), dout(R * sizeof(SampleOutEx)), db(NB * W * 4), dtok(64 * 4);
        std::vector<SampleRowEx> tab(R);
        for (size_t r = 0; r < R; r++) {
            SampleRow &b = tab[r].base;
            memcpy(&b.pen, rows + 8 * r, sizeof(PenRow));
            b.allowed = bitmap_of_row[r] < 0 ? nullptr : db.as<unsigned>() + (size_t)bitmap_of_row[r] * W;
            b.temp = temp_top_p[2 * r]; b.top_p = temp_top_p[2 * r + 1]; b.top_k = top_k[r]; b.tok_index = tok_index[r];
            b.seed = seed_draws[2 * r]; b.draws = seed_draws[2 * r + 1];
            const float *c = chain + 6 * r;
            tab[r].chain = ChainParams{c[0], c[1], c[2], mirostat[r], c[3], c[4], c[5], 0};
        }
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dr.p, tab.data(), R * sizeof(SampleRowEx), hipMemcpyHostToDevice));
        if (n_bitmaps > 0) HIP_CHECK(hipMemcpy(db.p, bitmaps, (size_t)n_bitmaps * W * 4, hipMemcpyHostToDevice));
        if (n_table > 0) HIP_CHECK(hipMemcpy(dt.p, table, (size_t)n_table * sizeof(PenEntry), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dtok.p, row_tok_io, 64 * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0xFF, R * sizeof(SampleOutEx)));                            // what the kernel leaves out shows as -1 / NaN
        if (!timed(ms_out, [&] { return launch_sample_rows_ex(dl.as<float>(), ld, n_vocab, n_rows, dr.as<SampleRowEx>(), dt.as<PenEntry>(), dout.as<SampleOutEx>(), dtok.as<int>(), nullptr); })) return 3;
        HIP_CHECK(hipMemcpy(out, dout.p, R * sizeof(SampleOutEx), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(row_tok_io, dtok.p, 64 * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// ---- speculation under sampling (draft_host.hpp, launch_draft_sample_finish) ----
// The sampled verify pass's epilogue alone: k_sample_rows over the R rows of host logits [R][ld], then k_draft_sample_finish on a two-slot state.  Everything that indexes
// device memory is checked here.
int minigpt4_amd_test_draft_sample(const float *logits, int R, int n_vocab, int ld, const int32_t *rows, const int32_t *table, int n_table, const uint32_t *bitmaps, int n_bitmaps,
                                   const int32_t *bitmap_of_row, const float *temp_top_p, const int32_t *top_k, const uint64_t *seed_draws, const int32_t *row_tok, int slot,
                                   int32_t *state_io, float *slot_logits_io, int32_t *res_out, int32_t *out, float *ms_out) {
    static_assert(sizeof(PenRow) == 32 && sizeof(PenEntry) == 16 && sizeof(SampleRow) == 72 && sizeof(SampleOut) == (5 + 2 * SAMPLE_MAX) * 4, "the hook's word layout");
    if (!logits || !rows || !bitmap_of_row || !temp_top_p || !top_k || !seed_draws || !row_tok || !state_io || !slot_logits_io || !res_out || !out || R < 1 || R > DRAFT_ROWS ||
        n_vocab < 1 || ld < n_vocab || slot < 0 || slot > 1 || n_table < 0 || (n_table > 0 && !table) || n_bitmaps < 0 || (n_bitmaps > 0 && !bitmaps)) return 1;
    if (!pen_rows_ok(rows, R, table, n_table, /*buf_rows=*/R, n_vocab)) return 1;
    for (int r = 0; r < R; r++) {   // row r decides on logits row r
        if (rows[8 * (size_t)r] != r || bitmap_of_row[r] < -1 || bitmap_of_row[r] >= n_bitmaps || top_k[r] < 1 || top_k[r] > std::min(SAMPLE_MAX, n_vocab)) return 1;
        const float temp = temp_top_p[2 * (size_t)r], top_p = temp_top_p[2 * (size_t)r + 1];
        if (!std::isfinite(temp) || !(temp > 0.0f) || !(top_p > 0.0f) || !(top_p <= 1.0f)) return 1;
    }
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)R * ld, T = (size_t)std::max(n_table, 1), W = (size_t)constraint_words(n_vocab), NB = (size_t)std::max(n_bitmaps, 1), V = (size_t)n_vocab;
        DevBuf dl(n * 4), dr((size_t)R * sizeof(SampleRow)), dt(T * sizeof(PenEntry)), dout((size_t)R * sizeof(SampleOut)), db(NB * W * 4), dtok(DRAFT_ROWS * 4), dslot(4), dst(6 * 4),
               dkeep(2 * V * 4), dres(DRAFT_SAMPLE_RES * 4);
        std::vector<SampleRow> tab((size_t)R);
        for (size_t r = 0; r < (size_t)R; r++) {
            memcpy(&tab[r].pen, rows + 8 * r, sizeof(PenRow));
            tab[r].allowed = bitmap_of_row[r] < 0 ? nullptr : db.as<unsigned>() + (size_t)bitmap_of_row[r] * W;
            tab[r].temp = temp_top_p[2 * r]; tab[r].top_p = temp_top_p[2 * r + 1]; tab[r].top_k = top_k[r]; tab[r].tok_index = -1;
            tab[r].seed = seed_draws[2 * r]; tab[r].draws = seed_draws[2 * r + 1];
        }
        int tok[DRAFT_ROWS]; for (int r = 0; r < DRAFT_ROWS; r++) tok[r] = r < R ? row_tok[r] : -1;
        // the state as the engine keeps it: n_past[2] | argmax[2] | feed[2]; the caller's layout is per slot (n_past, argmax, feed)
        int st[6]; for (int s = 0; s < 2; s++) for (int f = 0; f < 3; f++) st[2 * f + s] = state_io[3 * s + f];
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dr.p, tab.data(), (size_t)R * sizeof(SampleRow), hipMemcpyHostToDevice));
        if (n_bitmaps > 0) HIP_CHECK(hipMemcpy(db.p, bitmaps, (size_t)n_bitmaps * W * 4, hipMemcpyHostToDevice));
        if (n_table > 0) HIP_CHECK(hipMemcpy(dt.p, table, (size_t)n_table * sizeof(PenEntry), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dtok.p, tok, sizeof(tok), hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dslot.p, &slot, 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dst.p, st, sizeof(st), hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dkeep.p, slot_logits_io, 2 * V * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0xFF, (size_t)R * sizeof(SampleOut))); HIP_CHECK(hipMemset(dres.p, 0xFF, DRAFT_SAMPLE_RES * 4));   // what the kernels leave out shows as -1
        if (!launch_sample_rows(dl.as<float>(), ld, n_vocab, R, dr.as<SampleRow>(), dt.as<PenEntry>(), dout.as<SampleOut>(), nullptr, nullptr)) return 3;
        if (!timed(ms_out, [&] {                                                 // k_draft_sample_finish alone
                return launch_draft_sample_finish(dl.as<float>(), ld, n_vocab, R, dtok.as<int>(), dout.as<SampleOut>(), dslot.as<int>(), dst.as<int>(), dst.as<int>() + 2,
                                                  dst.as<int>() + 4, dkeep.as<float>(), dres.as<int>(), nullptr);
            })) return 3;
        HIP_CHECK(hipMemcpy(out, dout.p, (size_t)R * sizeof(SampleOut), hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(res_out, dres.p, DRAFT_SAMPLE_RES * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(st, dst.p, sizeof(st), hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(slot_logits_io, dkeep.p, 2 * V * 4, hipMemcpyDeviceToHost));
        for (int s = 0; s < 2; s++) for (int f = 0; f < 3; f++) state_io[3 * s + f] = st[2 * f + s];
        return 0;
    });
}
// draft_stage alone, no GPU
int minigpt4_amd_test_draft_tables(const int32_t *hist, int n_hist, int32_t x0, const int32_t *draft, int n_draft, int32_t repeat_last_n, float repeat_penalty, float alpha_presence,
                                   float alpha_frequency, int penalize_nl, const int32_t *bias_id, const float *bias_val, int n_bias, int n_ctx, int n_vocab, const uint16_t *trans,
                                   const uint32_t *accept, int n_states, int state, const uint8_t *vocab, const int32_t *off, int32_t *n_rows_out, int32_t *cut_out,
                                   int32_t *rows_out, int32_t *table_out, int table_cap, int32_t *n_table_out, int32_t *states_out) {
    if (n_hist < 0 || (n_hist > 0 && !hist) || n_draft < 0 || n_draft > DRAFT_ROWS - 1 || (n_draft > 0 && !draft) || n_bias < 0 || n_bias > PEN_BIAS_MAX ||
        (n_bias > 0 && (!bias_id || !bias_val)) || n_ctx < 1 || n_vocab < 1 || x0 < 0 || x0 >= n_vocab || !n_rows_out || !cut_out || !rows_out || !table_out || table_cap < 0 ||
        !n_table_out || !states_out) return 1;
    for (int i = 0; i < n_draft; i++) if (draft[i] < 0 || draft[i] >= n_vocab) return 1;
    for (int i = 0; i < n_bias; i++) if (bias_id[i] < 0 || bias_id[i] >= n_vocab) return 1;
    ConstraintDfa dfa;
    if (trans) {
        if (!accept || !vocab || !off || n_states < 2 || n_states > CONSTRAINT_MAX_STATES || state < 0 || state >= n_states) return 1;
        for (size_t i = 0; i < (size_t)n_states * 256; i++) if (trans[i] >= n_states) return 1;
        for (int i = 0; i < n_vocab; i++) if (off[i] < 0 || off[i + 1] < off[i]) return 1;
        dfa.n_states = n_states; dfa.trans.assign(trans, trans + (size_t)n_states * 256); dfa.accept.assign(accept, accept + ((size_t)n_states + 31) / 32);
    }
    auto piece = [&](int id, const unsigned char **b, int *n) { if (id < 0 || id >= n_vocab) return false; *b = vocab + off[id]; *n = off[id + 1] - off[id]; return true; };
    const PenParams pp{repeat_last_n, repeat_penalty, alpha_presence, alpha_frequency, penalize_nl};
    DraftStage st;
    draft_stage(hist, (size_t)n_hist, x0, draft, n_draft, pp, bias_id, bias_val, n_bias, n_ctx, n_vocab, trans ? &dfa : nullptr, state, piece, st);
    *n_rows_out = st.n_rows; *cut_out = st.cut; *n_table_out = (int)st.entries.size();
    if ((int)st.entries.size() > table_cap) return 4;
    memcpy(rows_out, st.rows.data(), st.rows.size() * sizeof(PenRow));
    memcpy(table_out, st.entries.data(), st.entries.size() * sizeof(PenEntry));
    for (int r = 0; r < st.n_rows; r++) states_out[r] = st.state[(size_t)r];
    return 0;
}
// ---- packed prompt rows of several conversations (Engine::prefill_batch) ----
// [n_seg][3] (slot, rows, pos0) -> the engine's device table [n_seg][4] (slot, first packed row, rows, pos0); false on a segment outside the caches
static bool seg_table(int n_ctx, int n_slots, int n_seg, const int32_t *segs, std::vector<int> &out, int &N, int &t_max) {
    out.assign((size_t)n_seg * 4, 0); N = 0; t_max = 0;
    for (int i = 0; i < n_seg; i++) {
        const int slot = segs[3 * i], rows = segs[3 * i + 1], pos0 = segs[3 * i + 2];
        if (slot < 0 || slot >= n_slots || rows < 1 || pos0 < 0 || pos0 + rows > n_ctx) return false;
        out[4 * (size_t)i] = slot; out[4 * (size_t)i + 1] = N; out[4 * (size_t)i + 2] = rows; out[4 * (size_t)i + 3] = pos0;
        N += rows; t_max = std::max(t_max, pos0 + rows);
    }
    return true;
}
int minigpt4_amd_test_attn_prefill_seg(int n_head, int hd, int n_ctx, int n_slots, const uint16_t *kc, const uint16_t *vc, int n_seg, const int32_t *segs, const float *q,
                                       int form, float *out_seg, float *out_ref, int *seg_launched, uint16_t *out_h_seg, uint16_t *out_h_ref, int *wrote_h) {
    std::vector<int> st; int N = 0, t_max = 0;
    if (!kc || !vc || !segs || !q || !out_seg || !out_ref || n_head < 1 || !attn_head_size_supported(hd) || n_slots < 1 || n_seg < 1 || form < 0 || form > 4 ||
        !seg_table(n_ctx, n_slots, n_seg, segs, st, N, t_max) || (!out_h_seg) != (!out_h_ref) || (out_h_seg && !wrote_h)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t E = (size_t)n_head * hd, cache = (size_t)n_slots * n_ctx * E, stride = (size_t)n_ctx * E;
        std::vector<int> t16((size_t)2 * (N + n_seg)), t32((size_t)2 * (N + n_seg));
        AttnSegs sg;
        sg.n_tiles[0] = attn_seg_tiles(st.data(), n_seg, 16, t16.data()); sg.n_tiles[1] = attn_seg_tiles(st.data(), n_seg, 32, t32.data());
        sg.t_max = t_max; sg.seq_stride = stride;
        DevBuf dk(cache * 2), dv(cache * 2), dq((size_t)N * E * 4), ds(st.size() * 4), d16(t16.size() * 4), d32(t32.size() * 4), da((size_t)N * E * 4), db((size_t)N * E * 4), dtab(65536 * 2);
        const bool want_h = out_h_seg != nullptr;                           // fp16 rows for an F16 wo (the out_h arm of the launchers)
        DevBuf dha(want_h ? (size_t)N * E * 2 : 0), dhb(want_h ? (size_t)N * E * 2 : 0);
        if (want_h) { HIP_CHECK(hipMemset(dha.p, 0, (size_t)N * E * 2)); HIP_CHECK(hipMemset(dhb.p, 0, (size_t)N * E * 2)); }
        HIP_CHECK(hipMemcpy(dk.p, kc, cache * 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, vc, cache * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dq.p, q, (size_t)N * E * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(ds.p, st.data(), st.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d16.p, t16.data(), t16.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(d32.p, t32.data(), t32.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(da.p, 0, (size_t)N * E * 4)); HIP_CHECK(hipMemset(db.p, 0, (size_t)N * E * 4));
        { std::vector<__half> e(65536); for (int i = 0; i < 65536; i++) e[(size_t)i] = __float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)i)))); HIP_CHECK(hipMemcpy(dtab.p, e.data(), 131072, hipMemcpyHostToDevice)); }
        Tables tb; tb.exp = dtab.as<__half>();
        { int nneg = 0; for (int c = 0x8000; c < 0xFC00; c++) { if (__half2float(__float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)c))))) == 0.0f) break; nneg++; } tb.exp_neg_n = (nneg + 2047) / 2048 * 2048; }
        sg.segs = ds.as<int>(); sg.tiles[0] = d16.as<int>(); sg.tiles[1] = d32.as<int>();
        LaunchTuning tune = hook_tuning();
        tune.attn_prefill_f16 = form != 4; tune.attn_prefill_form = form;   // (normalised: a form outside 1 .. 3 is the size rule)
        tune = tune.normalised();
        const float *dqp = dq.as<float>();
        // one launch_attn_prefill per segment; *all_h: every segment stored fp16 rows
        auto per_segment = [&](float *out, __half *out_h, bool *all_h) {
            if (all_h) *all_h = true;
            for (int i = 0; i < n_seg; i++) {
                const int *g = st.data() + 4 * (size_t)i;
                const size_t off = (size_t)g[1] * E, cs = (size_t)g[0] * stride;
                bool w = false;
                if (!launch_attn_prefill(dqp + off, dk.as<__half>() + cs, dv.as<__half>() + cs, g[2], n_head, hd, ds.as<int>() + 4 * i + 3, g[3] + g[2], tb, out + off, tune, nullptr,
                                         out_h ? out_h + off : nullptr, &w)) return false;
                if (all_h) *all_h = *all_h && w;
            }
            return true;
        };
        bool seg_h = false, ref_h = false;
        const bool one = launch_attn_prefill_seg(dqp, dk.as<__half>(), dv.as<__half>(), sg, n_head, hd, tb, da.as<float>(), tune, nullptr, want_h ? dha.as<__half>() : nullptr, &seg_h);
        if (!one && !per_segment(da.as<float>(), want_h ? dha.as<__half>() : nullptr, &seg_h)) return 4;
        if (!per_segment(db.as<float>(), want_h ? dhb.as<__half>() : nullptr, &ref_h)) return 4;
        HIP_CHECK(hipDeviceSynchronize());
        if (seg_launched) *seg_launched = one ? 1 : 0;
        HIP_CHECK(hipMemcpy(out_seg, da.p, (size_t)N * E * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(out_ref, db.p, (size_t)N * E * 4, hipMemcpyDeviceToHost));
        if (want_h) {
            wrote_h[0] = seg_h; wrote_h[1] = ref_h;
            HIP_CHECK(hipMemcpy(out_h_seg, dha.p, (size_t)N * E * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(out_h_ref, dhb.p, (size_t)N * E * 2, hipMemcpyDeviceToHost));
        }
        return 0;
    });
}
int minigpt4_amd_test_attn_draft(int mode, int n_head, int hd, int n_ctx, int n_slot, int slot, int n_past, int R, int computed_exp, const float *q, const float *k, const float *v,
                                 uint16_t *kc, uint16_t *vc, float *out) {
    if (!q || !k || !v || !kc || !vc || !out || (mode != 0 && mode != 1) || (hd != 32 && hd != 64 && hd != 128) || n_head < 1 || n_slot < 1 || slot < 0 || slot >= n_slot ||
        R < 1 || R > DRAFT_ROWS || n_past < 0 || n_ctx < 1 || n_past > n_ctx - R || n_ctx > attn_draft_max_ctx(hd)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t E = (size_t)n_head * hd, stride = (size_t)n_ctx * E, cache = (size_t)n_slot * stride, RE = (size_t)R * E;
        std::vector<float> c, sn;
        rope_tables(n_ctx, hd, c, sn);
        std::vector<int> np((size_t)n_slot, 0); np[(size_t)slot] = n_past;
        DevBuf dc(c.size() * 4), dsn(sn.size() * 4), dq(RE * 4), dk(RE * 4), dv(RE * 4), dkc(cache * 2), dvc(cache * 2), dout(RE * 4), dnp((size_t)n_slot * 4), dslot(4), dtab(65536 * 2);
        HIP_CHECK(hipMemcpy(dc.p, c.data(), c.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dsn.p, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dq.p, q, RE * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dk.p, k, RE * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, v, RE * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dkc.p, kc, cache * 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dvc.p, vc, cache * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dnp.p, np.data(), np.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dslot.p, &slot, 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0, RE * 4));
        // the engine's tables (Engine::alloc_buffers): the host libm's fp16 exp table and its live negative part; the decode step's copy has no table when it computes
        Tables tb;
        { std::vector<__half> e(65536); int last = 0;
          for (int i = 0; i < 65536; i++) e[(size_t)i] = __float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)i))));
          for (int i = 0; i < 0x7C00; i++) if (__half2float(e[(size_t)(0x8000 + i)]) != 0.0f) last = i;
          HIP_CHECK(hipMemcpy(dtab.p, e.data(), 131072, hipMemcpyHostToDevice));
          tb.exp = computed_exp ? nullptr : dtab.as<__half>(); tb.exp_neg_n = (last + 1 + 2047) / 2048 * 2048; }
        if (mode == 0) {
            launch_attn_llm_draft(dq.as<float>(), dk.as<float>(), dv.as<float>(), dkc.as<__half>(), dvc.as<__half>(), R, n_head, hd, dnp.as<int>(), dslot.as<int>(), stride, n_ctx,
                                  dc.as<float>(), dsn.as<float>(), tb, dout.as<float>(), nullptr);
        } else {
            for (int r = 0; r < R; r++) {
                launch_set_int(dnp.as<int>() + slot, n_past + r, nullptr);
                launch_attn_llm_batched(dq.as<float>() + (size_t)r * E, dk.as<float>() + (size_t)r * E, dv.as<float>() + (size_t)r * E, dkc.as<__half>(), dvc.as<__half>(), 1, n_head, hd,
                                        dnp.as<int>(), dslot.as<int>(), stride, n_ctx, dc.as<float>(), dsn.as<float>(), tb, dout.as<float>() + (size_t)r * E, nullptr);
            }
        }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, dout.p, RE * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(kc, dkc.p, cache * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(vc, dvc.p, cache * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}
int minigpt4_amd_test_attn_vsplit(int form, int vs, int n_head, int hd, int n_ctx, int n_slot, int rows, const int32_t *row_slot, const int32_t *n_past, int computed_exp,
                                  const float *q, const float *k, const float *v, uint16_t *kc, uint16_t *vc, float *out) {
    if (!q || !k || !v || !kc || !vc || !out || !row_slot || !n_past || form < 0 || form > 2 || (hd != 32 && hd != 64 && hd != 128) || !attn_vsplit_ok(hd, vs) || n_head < 1 ||
        n_slot < 1 || rows < 1 || n_ctx < 1 || n_ctx > (form == 2 ? attn_draft_max_ctx(hd) : attn_max_ctx(hd)) || (form == 0 && (rows != 1 || n_slot != 1)) ||
        (form == 2 && rows > DRAFT_ROWS)) return 1;
    // form 1: every row its own conversation; form 2: all rows in row_slot[0] at consecutive positions; every position written must lie inside the cache
    for (int r = 0; r < (form == 2 ? 1 : rows); r++) {
        if (row_slot[r] < 0 || row_slot[r] >= n_slot) return 1;
        for (int r2 = 0; r2 < r; r2++) if (row_slot[r2] == row_slot[r]) return 1;
        const int np = n_past[row_slot[r]];
        if (np < 0 || np > n_ctx - (form == 2 ? rows : 1)) return 1;
    }
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t E = (size_t)n_head * hd, stride = (size_t)n_ctx * E, cache = (size_t)n_slot * stride, RE = (size_t)rows * E;
        std::vector<float> c, sn;
        rope_tables(n_ctx, hd, c, sn);
        DevBuf dc(c.size() * 4), dsn(sn.size() * 4), dq(RE * 4), dk(RE * 4), dv(RE * 4), dkc(cache * 2), dvc(cache * 2), dout(RE * 4), dnp((size_t)n_slot * 4), dslot((size_t)rows * 4),
            dtab(65536 * 2);
        HIP_CHECK(hipMemcpy(dc.p, c.data(), c.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dsn.p, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dq.p, q, RE * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dk.p, k, RE * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, v, RE * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dkc.p, kc, cache * 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dvc.p, vc, cache * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dnp.p, n_past, (size_t)n_slot * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dslot.p, row_slot, (size_t)rows * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0, RE * 4));
        Tables tb;                                                // as in minigpt4_amd_test_attn_draft
        { std::vector<__half> e(65536); int last = 0;
          for (int i = 0; i < 65536; i++) e[(size_t)i] = __float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)i))));
          for (int i = 0; i < 0x7C00; i++) if (__half2float(e[(size_t)(0x8000 + i)]) != 0.0f) last = i;
          HIP_CHECK(hipMemcpy(dtab.p, e.data(), 131072, hipMemcpyHostToDevice));
          tb.exp = computed_exp ? nullptr : dtab.as<__half>(); tb.exp_neg_n = (last + 1 + 2047) / 2048 * 2048; }
        if (form == 0)
            launch_attn_llm(dq.as<float>(), dk.as<float>(), dv.as<float>(), dkc.as<__half>(), dvc.as<__half>(), 1, n_head, hd, dnp.as<int>(), n_ctx, dc.as<float>(), dsn.as<float>(), tb,
                            dout.as<float>(), true, nullptr, vs);
        else if (form == 1)
            launch_attn_llm_batched(dq.as<float>(), dk.as<float>(), dv.as<float>(), dkc.as<__half>(), dvc.as<__half>(), rows, n_head, hd, dnp.as<int>(), dslot.as<int>(), stride, n_ctx,
                                    dc.as<float>(), dsn.as<float>(), tb, dout.as<float>(), nullptr, vs);
        else
            launch_attn_llm_draft(dq.as<float>(), dk.as<float>(), dv.as<float>(), dkc.as<__half>(), dvc.as<__half>(), rows, n_head, hd, dnp.as<int>(), dslot.as<int>(), stride, n_ctx,
                                  dc.as<float>(), dsn.as<float>(), tb, dout.as<float>(), nullptr, vs);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, dout.p, RE * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(kc, dkc.p, cache * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(vc, dvc.p, cache * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}
// The two attention paths no other hook reaches, on ONE conversation's caches kc / vc [n_ctx][n_head * hd] (fp16 bit patterns, changed in place); q, k, v [rows][E] fp32 raw
// projections.  mode 0: `rows` successive decode steps through launch_attn_llm_split on ONE workspace -- filled with 0xFF bytes, then its last 1 KiB + n_head words zeroed,
// once, before the first step -- step i at position n_past + i.  mode 1: launch_rope_kv of the rows at n_past .. n_past + rows - 1, then launch_attn_llm(fused = false);
// q_rot [rows][E] receives the rotated q.  out [rows + 1][E]: prefilled with 0xFF bytes, the last row is a guard.
int minigpt4_amd_test_attn_rows(int mode, int n_head, int hd, int n_ctx, int n_past, int rows, int splits, int computed_exp, const float *q, const float *k, const float *v,
                                uint16_t *kc, uint16_t *vc, float *q_rot, float *out) {
    if (!q || !k || !v || !kc || !vc || !out || (mode != 0 && mode != 1) || (hd != 32 && hd != 64 && hd != 128) || n_head < 1 || n_head > 64 || rows < 1 || rows > 64 || n_past < 0 ||
        n_ctx < 1 || n_past > n_ctx - rows || n_ctx > attn_max_ctx(hd) || (mode == 0 && (splits < 2 || splits > 16)) || (mode == 1 && !q_rot)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t E = (size_t)n_head * hd, cache = (size_t)n_ctx * E, RE = (size_t)rows * E, GE = RE + E;
        std::vector<float> c, sn;
        rope_tables(n_ctx, hd, c, sn);
        const size_t ws_bytes = mode == 0 ? attn_split_workspace_bytes(n_head, hd, n_ctx, splits) : 16, ws_zero = 1024 + (size_t)n_head * 4;
        DevBuf dc(c.size() * 4), dsn(sn.size() * 4), dq(RE * 4), dk(RE * 4), dv(RE * 4), dkc(cache * 2), dvc(cache * 2), dout(GE * 4), dnp(4), dtab(65536 * 2), dws(ws_bytes);
        HIP_CHECK(hipMemcpy(dc.p, c.data(), c.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dsn.p, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dq.p, q, RE * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dk.p, k, RE * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, v, RE * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dkc.p, kc, cache * 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dvc.p, vc, cache * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dnp.p, &n_past, 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0xFF, GE * 4));
        Tables tb;                                                // as in minigpt4_amd_test_attn_draft
        { std::vector<__half> e(65536); int last = 0;
          for (int i = 0; i < 65536; i++) e[(size_t)i] = __float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)i))));
          for (int i = 0; i < 0x7C00; i++) if (__half2float(e[(size_t)(0x8000 + i)]) != 0.0f) last = i;
          HIP_CHECK(hipMemcpy(dtab.p, e.data(), 131072, hipMemcpyHostToDevice));
          tb.exp = computed_exp ? nullptr : dtab.as<__half>(); tb.exp_neg_n = (last + 1 + 2047) / 2048 * 2048; }
        if (mode == 0) {
            HIP_CHECK(hipMemset(dws.p, 0xFF, ws_bytes));
            HIP_CHECK(hipMemset(static_cast<unsigned char *>(dws.p) + (ws_bytes - ws_zero), 0, ws_zero));   // the arrival counters: once, never between the steps
            for (int i = 0; i < rows; i++) {
                if (i) launch_set_int(dnp.as<int>(), n_past + i, nullptr);
                launch_attn_llm_split(dq.as<float>() + (size_t)i * E, dk.as<float>() + (size_t)i * E, dv.as<float>() + (size_t)i * E, dkc.as<__half>(), dvc.as<__half>(), n_head, hd,
                                      dnp.as<int>(), n_ctx, dc.as<float>(), dsn.as<float>(), tb, dout.as<float>() + (size_t)i * E, dws.p, splits, nullptr);
            }
        } else {
            launch_rope_kv(dq.as<float>(), dk.as<float>(), dv.as<float>(), rows, n_head, hd, dnp.as<int>(), dc.as<float>(), dsn.as<float>(), dkc.as<__half>(), dvc.as<__half>(), nullptr);
            launch_attn_llm(dq.as<float>(), dk.as<float>(), dv.as<float>(), dkc.as<__half>(), dvc.as<__half>(), rows, n_head, hd, dnp.as<int>(), n_ctx, dc.as<float>(), dsn.as<float>(), tb,
                            dout.as<float>(), false, nullptr);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, dout.p, GE * 4, hipMemcpyDeviceToHost));
        if (q_rot) HIP_CHECK(hipMemcpy(q_rot, dq.p, RE * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(kc, dkc.p, cache * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(vc, dvc.p, cache * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}
int minigpt4_amd_test_ngram_draft(const int32_t *history, int n, int ngram_max, int ngram_min, int n_draft, int32_t *out) {
    if (n < 0 || (n > 0 && !history) || !out || ngram_min < 1 || ngram_max < ngram_min || n_draft < 0) return -1;
    NgramDrafter d(ngram_max, ngram_min);
    d.reset(history, n);
    return d.draft(n_draft, out);
}
// ---- the greedy step epilogues alone (llm_kernels.hip: launch_argmax / _advance, launch_batch_begin / _finish, launch_gather_rows / _seg_finish, launch_draft_begin / _finish) ----
// THE RULE every one of them follows ("first maximum wins"): the id is the lowest index i with row[i] equal to the maximum over the row's non-NaN entries, when that
// maximum is above -inf; otherwise (every entry NaN or -inf) it is 0.  The kernels reach it by a `v > best` sweep from best = -inf (false for a NaN, false for a second
// equal value: each thread keeps the first of its own), argmax_combine's "greater, or equal with the lower index" between threads, waves and workgroups, and the
// 0x7FFFFFFF "nothing seen" index that the last step turns into id 0.  tests/greedy_ref.py states the same rule in numpy.
// Every hook: plain host arrays in, every state array [n_slot + 1] words / [n_slot + 1][n_vocab] floats with the caller's guard behind the last slot, uploaded, returned
// after the launch.  Everything that indexes device memory is checked here, before a device is looked for.
static constexpr int SE_MAX_SLOTS = 4096, SE_MAX_VOCAB = 1 << 20;             // sanity caps of the hooks' allocations
static bool se_slots_ok(const int32_t *slots, int n, int stride, int n_slot) {   // n slots, `stride` words apart, each inside [0, n_slot) and named once
    std::vector<char> seen((size_t)n_slot, 0);
    for (int r = 0; r < n; r++) { const int s = slots[(size_t)r * stride]; if (s < 0 || s >= n_slot || seen[(size_t)s]) return false; seen[(size_t)s] = 1; }
    return true;
}
namespace {
// n_past | argmax | feed [n_slot + 1] each and the slots' logits rows [n_slot + 1][n_vocab] (n_vocab 0: none) on the device, from and back to the caller's arrays
struct StepState {
    size_t words, keep_bytes; DevBuf dn, da, df, dk;
    StepState(int n_slot, int n_vocab) : words((size_t)n_slot + 1), keep_bytes(words * (size_t)n_vocab * 4), dn(words * 4), da(words * 4), df(words * 4), dk(std::max<size_t>(keep_bytes, 4)) {}
    void upload(const int32_t *n_past, const int32_t *argmax, const int32_t *feed, const float *keep) {
        HIP_CHECK(hipMemcpy(dn.p, n_past, words * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(da.p, argmax, words * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(df.p, feed, words * 4, hipMemcpyHostToDevice));
        if (keep_bytes) HIP_CHECK(hipMemcpy(dk.p, keep, keep_bytes, hipMemcpyHostToDevice));
    }
    void download(int32_t *n_past, int32_t *argmax, int32_t *feed, float *keep) {
        HIP_CHECK(hipMemcpy(n_past, dn.p, words * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(argmax, da.p, words * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(feed, df.p, words * 4, hipMemcpyDeviceToHost));
        if (keep_bytes) HIP_CHECK(hipMemcpy(keep, dk.p, keep_bytes, hipMemcpyDeviceToHost));
    }
};
}
// ONE launch_argmax on logits[n] with the engine's 512-byte scratch (64 partial values, then 64 partial ids), prefilled with 0xFF bytes; the partials come back
int minigpt4_amd_test_argmax(const float *logits, int n, int32_t *out, float *partial_values_out, int32_t *partial_ids_out) {
    if (!logits || !out || n < 1 || n > (1 << 24)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        DevBuf dl((size_t)n * 4), ds(512), dout(2 * 4);                        // dout: the id and a guard word
        HIP_CHECK(hipMemcpy(dl.p, logits, (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(ds.p, 0xFF, 512)); HIP_CHECK(hipMemset(dout.p, 0xFF, 8));
        launch_argmax(dl.as<float>(), n, dout.as<int>(), ds.p, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        int32_t o[2]; HIP_CHECK(hipMemcpy(o, dout.p, 8, hipMemcpyDeviceToHost));
        if (o[1] != -1) { set_last_error("launch_argmax wrote behind its output word"); return 3; }
        *out = o[0];
        if (partial_values_out) HIP_CHECK(hipMemcpy(partial_values_out, ds.p, 256, hipMemcpyDeviceToHost));
        if (partial_ids_out) HIP_CHECK(hipMemcpy(partial_ids_out, static_cast<const char *>(ds.p) + 256, 256, hipMemcpyDeviceToHost));
        return 0;
    });
}
// form 0: ONE launch_batch_finish with row_slot[rows]; form 1: ONE launch_seg_finish with fin[rows][2] = (slot, new position)
int minigpt4_amd_test_step_finish(int form, const float *logits, int rows, int n_vocab, int n_slot, const int32_t *row_slot_or_fin, int32_t *n_past_io, int32_t *argmax_io,
                                  int32_t *feed_io, float *slot_logits_io) {
    if (!logits || !row_slot_or_fin || !n_past_io || !argmax_io || !feed_io || !slot_logits_io || (form != 0 && form != 1) || rows < 1 || rows > Engine::MAX_CONVERSATIONS ||
        n_vocab < 1 || n_vocab > SE_MAX_VOCAB || n_slot < rows || n_slot > SE_MAX_SLOTS) return 1;
    if (!se_slots_ok(row_slot_or_fin, rows, form == 0 ? 1 : 2, n_slot)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)rows * n_vocab, nd = (size_t)rows * (form == 0 ? 1 : 2);
        DevBuf dl(n * 4), dd(nd * 4);
        StepState st(n_slot, n_vocab);
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dd.p, row_slot_or_fin, nd * 4, hipMemcpyHostToDevice));
        st.upload(n_past_io, argmax_io, feed_io, slot_logits_io);
        if (form == 0) launch_batch_finish(dl.as<float>(), n_vocab, rows, dd.as<int>(), st.dn.as<int>(), st.da.as<int>(), st.df.as<int>(), st.dk.as<float>(), nullptr);
        else launch_seg_finish(dl.as<float>(), n_vocab, rows, dd.as<int>(), st.dn.as<int>(), st.da.as<int>(), st.df.as<int>(), st.dk.as<float>(), nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        st.download(n_past_io, argmax_io, feed_io, slot_logits_io);
        return 0;
    });
}
// ONE launch_draft_finish (both kernels).  res_out [1 + DRAFT_ROWS + 1]: the launcher's nine words prefilled with 0xFF bytes, and a guard word behind them
int minigpt4_amd_test_draft_finish(const float *logits, int R, int n_vocab, const int32_t *tok, int n_slot, int slot, int32_t *n_past_io, int32_t *argmax_io, int32_t *feed_io,
                                   float *slot_logits_io, int32_t *res_out) {
    if (!logits || !tok || !n_past_io || !argmax_io || !feed_io || !slot_logits_io || !res_out || R < 1 || R > DRAFT_ROWS || n_vocab < 1 || n_vocab > SE_MAX_VOCAB || n_slot < 1 ||
        n_slot > SE_MAX_SLOTS || slot < 0 || slot >= n_slot) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)R * n_vocab, NR = 1 + DRAFT_ROWS + 1;
        DevBuf dl(n * 4), dtok(DRAFT_ROWS * 4), dslot(4), dres(NR * 4);
        StepState st(n_slot, n_vocab);
        int t[DRAFT_ROWS]; for (int r = 0; r < DRAFT_ROWS; r++) t[r] = r < R ? tok[r] : -1;
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dtok.p, t, sizeof(t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dslot.p, &slot, 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemset(dres.p, 0xFF, NR * 4));
        st.upload(n_past_io, argmax_io, feed_io, slot_logits_io);
        launch_draft_finish(dl.as<float>(), n_vocab, R, dtok.as<int>(), dslot.as<int>(), st.dn.as<int>(), st.da.as<int>(), st.df.as<int>(), st.dk.as<float>(), dres.as<int>(), nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        st.download(n_past_io, argmax_io, feed_io, slot_logits_io);
        HIP_CHECK(hipMemcpy(res_out, dres.p, NR * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// The bookkeeping launches.  form 0: launch_advance on slot row_slot[0]'s words; 1: launch_batch_begin over n rows; 2: launch_draft_begin
int minigpt4_amd_test_step_words(int form, int n_slot, int n, const int32_t *row_slot, const int32_t *row_pos, int with_tok0, int32_t *n_past_io, int32_t *argmax_io,
                                 int32_t *feed_io) {
    if (!row_slot || !n_past_io || !argmax_io || !feed_io || form < 0 || form > 2 || n_slot < 1 || n_slot > SE_MAX_SLOTS) return 1;
    if (form != 0 && !row_pos) return 1;
    if (form == 1 && (n < 1 || n > Engine::MAX_CONVERSATIONS || n > n_slot)) return 1;
    const int B = form == 1 ? n : 1;
    if (!se_slots_ok(row_slot, B, 1, n_slot)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        DevBuf ds((size_t)B * 4), dp((size_t)B * 4);
        StepState st(n_slot, 0);
        HIP_CHECK(hipMemcpy(ds.p, row_slot, (size_t)B * 4, hipMemcpyHostToDevice));
        if (row_pos) HIP_CHECK(hipMemcpy(dp.p, row_pos, (size_t)B * 4, hipMemcpyHostToDevice));
        st.upload(n_past_io, argmax_io, feed_io, nullptr);
        const int slot = row_slot[0];
        if (form == 0) launch_advance(st.dn.as<int>() + slot, n, with_tok0 ? st.df.as<int>() + slot : nullptr, st.da.as<int>() + slot, nullptr);
        else if (form == 1) launch_batch_begin(st.dn.as<int>(), ds.as<int>(), dp.as<int>(), B, nullptr);
        else launch_draft_begin(st.dn.as<int>(), ds.as<int>(), dp.as<int>(), nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        st.download(n_past_io, argmax_io, feed_io, nullptr);
        return 0;
    });
}
// ---- the verify pass of several conversations: its attention launch and its prologue + epilogue alone ----
int minigpt4_amd_test_attn_draft_batch(int mode, int vs, int n_head, int hd, int n_ctx, int n_slot, int n_groups, const int32_t *groups, int computed_exp, const float *q,
                                       const float *k, const float *v, uint16_t *kc, uint16_t *vc, float *out) {
    if (!q || !k || !v || !kc || !vc || !out || !groups || (mode != 0 && mode != 1) || (hd != 32 && hd != 64 && hd != 128) || (vs != 1 && vs != 2 && vs != 4) || n_head < 1 ||
        n_slot < 1 || n_slot > SE_MAX_SLOTS || n_groups < 1 || n_groups > ATTN_MDRAFT_ROWS || n_ctx < 1 || n_ctx > attn_draft_max_ctx(hd)) return 1;
    if (!se_slots_ok(groups, n_groups, 3, n_slot)) return 1;
    int N = 0;
    for (int g = 0; g < n_groups; g++) {
        const int p0 = groups[3 * g + 1], R = groups[3 * g + 2];
        if (R < 1 || R > DRAFT_ROWS || p0 < 0 || p0 > n_ctx - R) return 1;
        N += R;
    }
    if (N > ATTN_MDRAFT_ROWS) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t E = (size_t)n_head * hd, stride = (size_t)n_ctx * E, cache = (size_t)n_slot * stride, RE = (size_t)N * E;
        std::vector<float> c, sn;
        rope_tables(n_ctx, hd, c, sn);
        std::vector<int> np((size_t)n_slot, 0), rs((size_t)N), rp((size_t)N), first((size_t)n_groups);
        for (int g = 0, t = 0; g < n_groups; g++) {
            first[(size_t)g] = t;
            if (mode == 1) np[(size_t)groups[3 * g]] = groups[3 * g + 1];    // mode 0: k_mdraft_begin writes them
            for (int r = 0; r < groups[3 * g + 2]; r++, t++) { rs[(size_t)t] = groups[3 * g]; rp[(size_t)t] = groups[3 * g + 1] + r; }
        }
        DevBuf dc(c.size() * 4), dsn(sn.size() * 4), dq(RE * 4), dk(RE * 4), dv(RE * 4), dkc(cache * 2), dvc(cache * 2), dout(RE * 4), dnp((size_t)n_slot * 4), dslot((size_t)N * 4),
            dpos((size_t)N * 4), dtab(65536 * 2);
        HIP_CHECK(hipMemcpy(dc.p, c.data(), c.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dsn.p, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dq.p, q, RE * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dk.p, k, RE * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, v, RE * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dkc.p, kc, cache * 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dvc.p, vc, cache * 2, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dnp.p, np.data(), np.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dslot.p, rs.data(), (size_t)N * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dpos.p, rp.data(), (size_t)N * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0, RE * 4));
        Tables tb;                                                // as in minigpt4_amd_test_attn_draft
        { std::vector<__half> e(65536); int last = 0;
          for (int i = 0; i < 65536; i++) e[(size_t)i] = __float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)i))));
          for (int i = 0; i < 0x7C00; i++) if (__half2float(e[(size_t)(0x8000 + i)]) != 0.0f) last = i;
          HIP_CHECK(hipMemcpy(dtab.p, e.data(), 131072, hipMemcpyHostToDevice));
          tb.exp = computed_exp ? nullptr : dtab.as<__half>(); tb.exp_neg_n = (last + 1 + 2047) / 2048 * 2048; }
        if (mode == 0) {
            launch_mdraft_begin(dnp.as<int>(), dslot.as<int>(), dpos.as<int>(), N, nullptr);
            launch_attn_llm_draft_batched(dq.as<float>(), dk.as<float>(), dv.as<float>(), dkc.as<__half>(), dvc.as<__half>(), N, n_head, hd, dnp.as<int>(), dslot.as<int>(), dpos.as<int>(),
                                          stride, n_ctx, dc.as<float>(), dsn.as<float>(), tb, dout.as<float>(), nullptr, vs);
        } else {
            for (int g = 0; g < n_groups; g++) {
                const size_t o = (size_t)first[(size_t)g] * E;
                launch_attn_llm_draft(dq.as<float>() + o, dk.as<float>() + o, dv.as<float>() + o, dkc.as<__half>(), dvc.as<__half>(), groups[3 * g + 2], n_head, hd, dnp.as<int>(),
                                      dslot.as<int>() + first[(size_t)g], stride, n_ctx, dc.as<float>(), dsn.as<float>(), tb, dout.as<float>() + o, nullptr, vs);
            }
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, dout.p, RE * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(kc, dkc.p, cache * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(vc, dvc.p, cache * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}
int minigpt4_amd_test_draft_finish_batch(const float *logits, int N, int n_vocab, const int32_t *tok, const int32_t *row_slot, const int32_t *row_pos, int n_slot, int32_t *n_past_io,
                                         int32_t *argmax_io, int32_t *feed_io, float *slot_logits_io, int32_t *res_out) {
    if (!logits || !tok || !row_slot || !row_pos || !n_past_io || !argmax_io || !feed_io || !slot_logits_io || !res_out || N < 1 || N > ATTN_MDRAFT_ROWS || n_vocab < 1 ||
        n_vocab > SE_MAX_VOCAB || n_slot < 1 || n_slot > SE_MAX_SLOTS) return 1;
    {   // consecutive groups: rows of one slot adjacent, at most DRAFT_ROWS of them, at consecutive positions
        std::vector<char> seen((size_t)n_slot, 0);
        for (int t = 0, run = 0; t < N; t++) {
            const int s = row_slot[t];
            if (s < 0 || s >= n_slot || row_pos[t] < 0) return 1;
            if (t > 0 && row_slot[t - 1] == s) { if (++run > DRAFT_ROWS || row_pos[t] != row_pos[t - 1] + 1) return 1; }
            else { if (seen[(size_t)s]) return 1; seen[(size_t)s] = 1; run = 1; }
        }
    }
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t n = (size_t)N * n_vocab, NR = 2 * ATTN_MDRAFT_ROWS + 1;
        DevBuf dl(n * 4), dtok((size_t)N * 4), dslot((size_t)N * 4), dpos((size_t)N * 4), dres(NR * 4);
        StepState st(n_slot, n_vocab);
        HIP_CHECK(hipMemcpy(dl.p, logits, n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dtok.p, tok, (size_t)N * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dslot.p, row_slot, (size_t)N * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dpos.p, row_pos, (size_t)N * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dres.p, 0xFF, NR * 4));
        st.upload(n_past_io, argmax_io, feed_io, slot_logits_io);
        launch_mdraft_begin(st.dn.as<int>(), dslot.as<int>(), dpos.as<int>(), N, nullptr);
        launch_draft_finish_batch(dl.as<float>(), n_vocab, N, dtok.as<int>(), dslot.as<int>(), st.dn.as<int>(), st.da.as<int>(), st.df.as<int>(), st.dk.as<float>(), dres.as<int>(), nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        st.download(n_past_io, argmax_io, feed_io, slot_logits_io);
        HIP_CHECK(hipMemcpy(res_out, dres.p, NR * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
// ONE launch_gather_rows: dst_out [n + 1][E], prefilled with 0xFF bytes, row n is a guard row
int minigpt4_amd_test_gather_rows(const float *src, int n_src, const int32_t *idx, int n, int E, float *dst_out) {
    if (!src || !idx || !dst_out || n_src < 1 || n_src > (1 << 16) || n < 1 || n > (1 << 16) || E < 1 || E > SE_MAX_VOCAB) return 1;
    for (int r = 0; r < n; r++) if (idx[r] < 0 || idx[r] >= n_src) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t ns = (size_t)n_src * E, nd = ((size_t)n + 1) * E;
        DevBuf dsrc(ns * 4), di((size_t)n * 4), dd(nd * 4);
        HIP_CHECK(hipMemcpy(dsrc.p, src, ns * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(di.p, idx, (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dd.p, 0xFF, nd * 4));
        launch_gather_rows(dsrc.as<float>(), di.as<int>(), n, E, dd.as<float>(), nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(dst_out, dd.p, nd * 4, hipMemcpyDeviceToHost));
        return 0;
    });
}
int minigpt4_amd_test_rope_kv_seg(int n_head, int hd, int n_ctx, int n_slots, int n_seg, const int32_t *segs, const float *q, const float *k, const float *v, int ks,
                                  float *q_seg, uint16_t *kc_seg, uint16_t *vc_seg, float *q_ref, uint16_t *kc_ref, uint16_t *vc_ref) {
    std::vector<int> st; int N = 0, t_max = 0;
    if (!segs || !q || !k || !v || !q_seg || !kc_seg || !vc_seg || !q_ref || !kc_ref || !vc_ref || n_head < 1 || hd < 2 || hd % 2 || n_slots < 1 || n_seg < 1 || ks < 1 || ks > 8 ||
        !seg_table(n_ctx, n_slots, n_seg, segs, st, N, t_max)) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const size_t E = (size_t)n_head * hd, cache = (size_t)n_slots * n_ctx * E, stride = (size_t)n_ctx * E, NE = (size_t)N * E;
        std::vector<float> c, sn;
        rope_tables(n_ctx, hd, c, sn);
        std::vector<int> rows((size_t)2 * N);
        for (int i = 0; i < n_seg; i++) for (int r = 0; r < st[4 * (size_t)i + 2]; r++) { rows[2 * (size_t)(st[4 * (size_t)i + 1] + r)] = st[4 * (size_t)i]; rows[2 * (size_t)(st[4 * (size_t)i + 1] + r) + 1] = st[4 * (size_t)i + 3] + r; }
        DevBuf dc(c.size() * 4), dsn(sn.size() * 4), ds(st.size() * 4), dr(rows.size() * 4), dslab(3 * (size_t)ks * NE * 4), dqa(NE * 4), dqb(NE * 4), dka(cache * 2), dva(cache * 2), dkb(cache * 2), dvb(cache * 2);
        HIP_CHECK(hipMemcpy(dc.p, c.data(), c.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dsn.p, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(ds.p, st.data(), st.size() * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dr.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        const float *src[3] = {q, k, v};
        for (int a = 0; a < 3; a++) for (int z = 0; z < ks; z++) HIP_CHECK(hipMemcpy(dslab.as<float>() + ((size_t)a * ks + z) * NE, src[a], NE * 4, hipMemcpyHostToDevice));   // slab z of matrix a
        for (DevBuf *b : {&dka, &dva, &dkb, &dvb}) HIP_CHECK(hipMemset(b->p, 0, cache * 2));
        HIP_CHECK(hipMemcpy(dqa.p, q, NE * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dqb.p, q, NE * 4, hipMemcpyHostToDevice));
        float *sl = dslab.as<float>();
        auto slabs = [&](size_t off, float *qout) {
            SlabSrc S; S.ws = sl; S.ks = ks; S.stride = (long long)NE; S.n = 3; S.y[0] = qout;
            for (int a = 0; a < 3; a++) { S.mbase[a] = sl + (size_t)a * ks * NE + off; S.mks[a] = ks; }
            return S;
        };
        // the plain forms read the first slab of k / v (= k, v); q is rotated in place in its own copy
        if (ks > 1) launch_rope_kv_seg_slabs(slabs(0, dqa.as<float>()), N, n_head, hd, dr.as<int>(), stride, dc.as<float>(), dsn.as<float>(), dka.as<__half>(), dva.as<__half>(), nullptr);
        else launch_rope_kv_seg(dqa.as<float>(), sl + NE, sl + 2 * NE, N, n_head, hd, dr.as<int>(), stride, dc.as<float>(), dsn.as<float>(), dka.as<__half>(), dva.as<__half>(), nullptr);
        for (int i = 0; i < n_seg; i++) {
            const int *g = st.data() + 4 * (size_t)i;
            const size_t off = (size_t)g[1] * E, cs = (size_t)g[0] * stride;
            const int *np = ds.as<int>() + 4 * i + 3;
            if (ks > 1) launch_rope_kv_slabs(slabs(off, dqb.as<float>() + off), g[2], n_head, hd, np, dc.as<float>(), dsn.as<float>(), dkb.as<__half>() + cs, dvb.as<__half>() + cs, nullptr);
            else launch_rope_kv(dqb.as<float>() + off, sl + NE + off, sl + 2 * NE + off, g[2], n_head, hd, np, dc.as<float>(), dsn.as<float>(), dkb.as<__half>() + cs, dvb.as<__half>() + cs, nullptr);
        }
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(q_seg, dqa.p, NE * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(q_ref, dqb.p, NE * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(kc_seg, dka.p, cache * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(vc_seg, dva.p, cache * 2, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(kc_ref, dkb.p, cache * 2, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(vc_ref, dvb.p, cache * 2, hipMemcpyDeviceToHost));
        return 0;
    });
}
// Micro-benchmark of the prompt-row attention (launch_attn_prefill): N query rows at positions n_past .. n_past + N - 1 of an fp16 K / V cache filled with synthetic rows
int minigpt4_amd_bench_attn_prefill(int n_head, int hd, int N, int n_past, int iters, float *us_per_launch) {
    if (n_head < 1 || !attn_head_size_supported(hd) || N < 2 || n_past < 0 || iters < 1) return 1;
    if (device_count_noexcept() <= 0) { set_last_error("no HIP device"); return 2; }
    return guarded(3, [&]() -> int {
        const int E = n_head * hd, T = n_past + N;
        DevBuf dq((size_t)N * E * 4), dk((size_t)T * E * 2), dv((size_t)T * E * 2), dout((size_t)N * E * 4), dtab(65536 * 2), dnp(4);
        { std::vector<float> h((size_t)N * E); for (size_t i = 0; i < h.size(); i++) h[i] = (float)((int)(i * 2654435761u % 2001u) - 1000) / 4000.0f; HIP_CHECK(hipMemcpy(dq.p, h.data(), h.size() * 4, hipMemcpyHostToDevice)); }
        { std::vector<__half> h((size_t)T * E); for (size_t i = 0; i < h.size(); i++) h[i] = __float2half_rn((float)((int)(i * 40503u % 1001u) - 500) / 500.0f);
          HIP_CHECK(hipMemcpy(dk.p, h.data(), h.size() * 2, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(dv.p, h.data(), h.size() * 2, hipMemcpyHostToDevice)); }
        { std::vector<__half> e(65536); for (int i = 0; i < 65536; i++) e[(size_t)i] = __float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)i)))); HIP_CHECK(hipMemcpy(dtab.p, e.data(), 131072, hipMemcpyHostToDevice)); }
        HIP_CHECK(hipMemcpy(dnp.p, &n_past, 4, hipMemcpyHostToDevice));
        Tables tb; tb.exp = dtab.as<__half>();
        { int nneg = 0; for (int c = 0x8000; c < 0xFC00; c++) { if (__half2float(__float2half_rn(expf(__half2float(__ushort_as_half((unsigned short)c))))) == 0.0f) break; nneg++; } tb.exp_neg_n = (nneg + 2047) / 2048 * 2048; }
        LaunchTuning tune = hook_tuning();
        if (const char *w8 = getenv("MINIGPT4_ATTN_PREFILL_W8")) tune.attn_prefill_w8 = atoi(w8);      // micro-benchmark only (no engine in this process)
        tune = tune.normalised();
        auto run = [&]() { return launch_attn_prefill(dq.as<float>(), dk.as<__half>(), dv.as<__half>(), N, n_head, hd, dnp.as<int>(), T, tb, dout.as<float>(), tune, nullptr); };
        for (int i = 0; i < 3; i++) if (!run()) return 4;
        HIP_CHECK(hipDeviceSynchronize());
        float ms = 0;
        timed(&ms, [&] { for (int i = 0; i < iters; i++) run(); return true; });
        if (us_per_launch) *us_per_launch = ms * 1e3f / (float)iters;
        return 0;
    });
}
int minigpt4_amd_timeline_attn(unsigned long long *out, int max_workgroups) { return (out && max_workgroups > 0) ? read_attn_timeline(out, max_workgroups) : -1; }
void minigpt4_amd_test_set_gemm_arm(int arm, int sk_arm) { g_tune.gemm_arm = arm; g_tune.gemm_sk_arm = sk_arm; g_tune = g_tune.normalised(); }
void minigpt4_amd_test_set_splitk_xcd(int on) { g_tune.splitk_xcd = on; g_tune = g_tune.normalised(); }
static int tuning_fields(const LaunchTuning &t, int *out, int n) {
    const int f[MINIGPT4_AMD_TUNING_FIELDS] = {t.cus, t.mv_waves_per_cu, t.mmq, t.mmqh, t.mmq_ks, t.mmq3_waves, t.attn_prefill_w8, t.attn_prefill_f16, t.attn_prefill_form, t.gemm_arm, t.gemm_sk_arm,
                                               t.f16_ks, t.splitk_xcd, t.attn_vit_qt};
    if (!out || n < 0) return -1;
    n = std::min(n, MINIGPT4_AMD_TUNING_FIELDS);
    std::copy(f, f + n, out);
    return n;
}
int minigpt4_amd_test_tuning_from_env(int cus, int *out, int n) { return tuning_fields(launch_tuning_from_env(cus), out, n); }
int minigpt4_amd_test_context_tuning(MiniGPT4Context *ctx, int *out, int n) { return ctx ? tuning_fields(E_(ctx)->launch_tuning(), out, n) : -1; }
int minigpt4_amd_timeline_vision(unsigned long long *out, int max_workgroups) { return (out && max_workgroups > 0) ? read_vision_timeline(out, max_workgroups) : -1; }

// Micro-benchmark of the decode mat-vec kernels on synthetic planes (random quant bytes, sane fp16 scales).  `n_sets` distinct weight sets
// are cycled so the 256 MiB Infinity Cache cannot serve repeats.  variant 0 = k_mul_mat per matrix, 1 = persistent-wave v2 (fused set).
int minigpt4_amd_bench_matvec(int ggml_type, int rows, int cols, int n_mat, int variant, int iters, int n_sets, int waves_per_cu, float *us_per_launch, double *bytes_per_launch) {
    if (!qweight_supported(ggml_type) || rows <= 0 || cols <= 0 || cols % gt_block(ggml_type) || n_mat < 1 || n_mat > 3 || iters < 1 || n_sets < 1) return 1;
    if (device_count_noexcept() <= 0) return 2;
    return guarded(3, [&]() -> int {
        LaunchTuning tune = hook_tuning(); tune.mv_waves_per_cu = waves_per_cu; tune = tune.normalised();
        QWeight plan; const size_t need = plan_qweight(ggml_type, rows, cols, plan, nullptr);
        std::vector<std::unique_ptr<DevBuf>> keep;
        std::vector<QWeight> W((size_t)n_sets * n_mat);
        for (size_t i = 0; i < W.size(); i++) {
            keep.emplace_back(new DevBuf(need));
            uint8_t *base = (uint8_t *)keep.back()->p;
            plan_qweight(ggml_type, rows, cols, W[i], base);
            launch_fill_random(base, need, (unsigned)(i * 7919 + 13), nullptr);
            const size_t n = (size_t)rows * cols;
            if (W[i].sc) { const size_t sc_bytes = (size_t)((W[i].d ? W[i].d : base + need) - W[i].sc);
                if (ggml_type == GT_Q4_K || ggml_type == GT_Q5_K) { /* header: d, dmin fp16 then 12 scale bytes: make d/dmin sane, keep scales random */
                    launch_fill_u16((void *)W[i].sc, std::min(sc_bytes, n / 256 * 16) / 2, 0x1C00, nullptr); }
                else if (ggml_type != GT_Q6_K) launch_fill_u16((void *)W[i].sc, std::min(sc_bytes, n / 32 * 4) / 2, 0x1C00, nullptr); }
            if (W[i].d) launch_fill_u16((void *)W[i].d, n / 256, 0x1C00, nullptr);
            if (ggml_type == GT_F16) launch_fill_u16(base, n, 0x2E66, nullptr);
            if (ggml_type == GT_F32) { std::vector<float> h(n, 0.01f); HIP_CHECK(hipMemcpy(base, h.data(), n * 4, hipMemcpyHostToDevice)); }
        }
        // variants 3..6: the batched decode's multi-row launch (weights streamed once): 3 = 4 prepared rows, 4 = 2 prepared rows, 5 = 2 rows prepared inside the launch, 6 = 4 rows inside
        // 10 + N / 20 + N: the multi-row launch with N = 1..4 prepared rows / rows prepared inside the launch (N = 1 and 3 run the 2- and 4-row kernels with a row to spare)
        const int NR = (variant > 10 && variant <= 14) ? variant - 10 : (variant > 20 && variant <= 24) ? variant - 20 : (variant == 3 || variant == 6) ? 4 : ((variant == 4 || variant == 5) ? 2 : 1);
        ActQ A; alloc_act(A, keep, (size_t)NR, (size_t)cols);
        DevBuf dx((size_t)NR * cols * 4), dy((size_t)rows * 4 * 3 * NR);
        { std::vector<float> hx((size_t)NR * cols); for (size_t i = 0; i < hx.size(); i++) hx[i] = (float)((int)(i * 37 % 201) - 100) / 64.0f; HIP_CHECK(hipMemcpy(dx.p, hx.data(), hx.size() * 4, hipMemcpyHostToDevice)); }
        launch_rms_quant(dx.as<float>(), nullptr, NR, cols, A, act_mask_for(ggml_type), nullptr);
        const bool issue_bar = getenv("MG4_MV_IB") && atoi(getenv("MG4_MV_IB")) != 0;   // issue barrier of the prologue variants (2, 7)
        auto run = [&](int set) {
            const QWeight *Wp[3]; float *Yp[3];
            for (int m = 0; m < n_mat; m++) { Wp[m] = &W[(size_t)set * n_mat + m]; Yp[m] = dy.as<float>() + (size_t)m * rows * NR; }
            if (variant == 7 && launch_matvec_set(Wp, Yp, Yp, n_mat, A, tune, nullptr, 2, dx.as<float>(), nullptr, nullptr, 0, issue_bar)) return;   // plain prologue + residual in place, as the decode's wo launch
            if (variant == 1 && launch_matvec_set(Wp, Yp, nullptr, n_mat, A, tune, nullptr)) return;
            if ((variant == 3 || variant == 4 || (variant > 10 && variant <= 14)) && launch_matvec_rows(Wp, Yp, nullptr, n_mat, A, NR, rows, tune, nullptr)) return;
            if ((variant == 5 || variant == 6 || (variant > 20 && variant <= 24)) && launch_matvec_rows(Wp, Yp, nullptr, n_mat, A, NR, rows, tune, nullptr, dx.as<float>(), dx.as<float>(), cols)) return;
            if (variant == 2 && launch_matvec_set(Wp, Yp, nullptr, n_mat, A, tune, nullptr, 1, dx.as<float>(), dx.as<float>(), nullptr, 0, issue_bar)) return;   // rms-norm prologue, as the decode's qkv / w1|w3 launches
            for (int m = 0; m < n_mat; m++) launch_mul_mat(*Wp[m], A, 1, Yp[m], rows, nullptr, tune, nullptr);
        };
        for (int i = 0; i < std::min(n_sets, 4); i++) run(i);
        HIP_CHECK(hipDeviceSynchronize());
        float ms = 0;
        timed(&ms, [&] { for (int i = 0; i < iters; i++) run(i % n_sets); return true; });
        if (us_per_launch) *us_per_launch = ms * 1e3f / (float)iters;
        if (bytes_per_launch) *bytes_per_launch = (double)gt_nbytes(ggml_type, (size_t)rows * cols) * n_mat;
        return 0;
    });
}

// Prefill mat-mul micro-benchmark (tools/mmq2_bench.py): n_mat matrices of random blocks against N random rows, `iters` launches of the engine's prefill launch
// (generation 2: mmq2_kernels.hip; generation 1: the round-1 kernels, one launch per matrix); ks: forced K split (0 = the launcher's choice).
int minigpt4_amd_bench_mmq(int ggml_type, int rows, int cols, int n_mat, int N, int iters, int ks, int generation, float *us_per_launch) {
    if (!qweight_supported(ggml_type) || rows <= 0 || cols <= 0 || cols % gt_block(ggml_type) || n_mat < 1 || n_mat > 3 || iters < 1 || N < 1) return 1;
    if (device_count_noexcept() <= 0) return 2;
    return guarded(3, [&]() -> int {
        QWeight plan; const size_t need = plan_qweight(ggml_type, rows, cols, plan, nullptr);
        std::vector<std::unique_ptr<DevBuf>> keep;
        QWeight W[3];
        for (int i = 0; i < n_mat; i++) {
            keep.emplace_back(new DevBuf(need));
            uint8_t *base = (uint8_t *)keep.back()->p;
            plan_qweight(ggml_type, rows, cols, W[i], base);
            launch_fill_random(base, need, (unsigned)(i * 7919 + 13), nullptr);
            const size_t n = (size_t)rows * cols;
            if (ggml_type == GT_Q4_K || ggml_type == GT_Q5_K) launch_fill_u16((void *)W[i].sc, n / 256 * 16 / 2, 0x1C00, nullptr);
            if (W[i].d) launch_fill_u16((void *)W[i].d, n / 256, 0x1C00, nullptr);
        }
        ActQ A; alloc_act(A, keep, (size_t)N, (size_t)cols);
        const size_t out_each = (size_t)N * rows;
        DevBuf dx((size_t)N * cols * 4), dy(out_each * n_mat * 4), dws(out_each * n_mat * 16 * 4);
        { std::vector<float> hx((size_t)N * cols); for (size_t i = 0; i < hx.size(); i++) hx[i] = (float)((int)(i * 37 % 201) - 100) / 64.0f; HIP_CHECK(hipMemcpy(dx.p, hx.data(), hx.size() * 4, hipMemcpyHostToDevice)); }
        launch_rms_quant(dx.as<float>(), nullptr, N, cols, A, act_mask_for(ggml_type), nullptr);
        A.ws = dws.as<float>(); A.ws_floats = out_each * n_mat * 16;
        LaunchTuning tune = hook_tuning();
        tune.mmq_ks = ks; tune.mmq = std::min(generation, 2); tune.mmqh = generation == 4;   // 4: the fp16-MFMA form of the Q4_K / Q5_K launches (k_mmqh_q45k), 2: the int8 kernels
        if (const char *e = getenv("MMQ3_NW")) tune.mmq3_waves = atoi(e);
        tune = tune.normalised();
        const uint8_t *Pp[3] = {nullptr, nullptr, nullptr};
        if (generation == 3) {
            if (!mmq3_supported(ggml_type, rows, cols)) return 4;
            const size_t pb = mmq3_plane_bytes(rows, cols);
            for (int i = 0; i < n_mat; i++) { keep.emplace_back(new DevBuf(pb)); Pp[i] = (const uint8_t *)keep.back()->p; launch_mmq3_build(W[i], (uint8_t *)keep.back()->p, nullptr); }
        }
        const QWeight *Wp[3]; float *Yp[3];
        for (int m = 0; m < n_mat; m++) { Wp[m] = &W[m]; Yp[m] = dy.as<float>() + (size_t)m * out_each; }
        auto run = [&]() {
            if (generation == 3) { if (!launch_mmq3_set(Wp, Pp, Yp, nullptr, n_mat, A, N, rows, tune, nullptr)) throw HipError{hipErrorInvalidValue, "mmq3 refused the shape", __FILE__, __LINE__}; return; }
            if (generation >= 2 && launch_mmq2_set(Wp, Yp, nullptr, n_mat, A, N, rows, tune, nullptr)) return;
            for (int m = 0; m < n_mat; m++) launch_mul_mat(*Wp[m], A, N, Yp[m], rows, nullptr, tune, nullptr);
        };
        run(); run();
        HIP_CHECK(hipDeviceSynchronize());
        float ms = 0;
        timed(&ms, [&] { for (int i = 0; i < iters; i++) run(); return true; });
        if (us_per_launch) *us_per_launch = ms * 1e3f / (float)iters;
        return 0;
    });
}

// Kernels of directions that were measured and closed (mmq3_kernels.hip: the digit-plane prompt mat-mul of round 4; tn_mfma_probe.hip: the batched-decode MFMA probe of round 5)
// are built into the test library only by `make test-extras` (-DMG4_TEST_EXTRAS); the default test library carries these refusing stubs, and minigpt4_amd_test_extras() says which.
#ifndef MG4_TEST_EXTRAS
extern "C++" {
namespace mg4 {
bool mmq3_supported(int, int, int) { return false; }
size_t mmq3_plane_bytes(int, int, size_t *) { return 0; }
void launch_mmq3_build(const QWeight &, uint8_t *, hipStream_t) {}
bool launch_mmq3_set(const QWeight *const *, const uint8_t *const *, float *const *, const float *const *, int, const ActQ &, int, int, const LaunchTuning &, hipStream_t, SlabSrc *) { return false; }
int probe_tn_mfma(int, int, int, int, int, int, int, float *, float *) { return 5; }
}
}  // extern "C++"
int minigpt4_amd_test_extras(void) { return 0; }
#else
int minigpt4_amd_test_extras(void) { return 1; }
#endif
int minigpt4_amd_probe_tn_mfma(int rows, int cols, int TN, int iters, int n_sets, int check, float *us_per_launch, float *rel_diff) {
    if (device_count_noexcept() <= 0) return 2;
    return guarded(3, [&]() -> int { hipDeviceProp_t prop; HIP_CHECK(hipGetDeviceProperties(&prop, 0)); return probe_tn_mfma(rows, cols, TN, iters, n_sets, check, prop.multiProcessorCount, us_per_launch, rel_diff); });
}
float minigpt4_amd_probe_valu(int op, int waves_per_simd, int iters) {
    if (device_count_noexcept() <= 0 || iters < 1) return -1.0f;
    float ns = -1.0f;
    guarded(1, [&] { hipDeviceProp_t prop; HIP_CHECK(hipGetDeviceProperties(&prop, 0)); ns = probe_valu_ns(op, waves_per_simd, iters, prop.multiProcessorCount); return 0; });
    return ns;
}
int minigpt4_amd_dist_env(int *world, int *rank, char *id_file, size_t cap, char *err, size_t err_cap) { return parse_dist_env_for_test(world, rank, id_file, cap, err, err_cap); }
float minigpt4_amd_probe_dma(int form, int policy, int waves, int fill, int depth, int deal, double total_gb) {
    float r = -1.0f;
    guarded(1, [&] { r = probe_dma_GBps(form, policy, waves, fill, depth, deal, (size_t)(total_gb * 1e9)); return 0; });
    return r;
}
float minigpt4_amd_probe_grid_barrier(int n_blocks, int iters, unsigned *errors) {
    if (n_blocks < 1 || n_blocks > 1024 || iters < 1 || device_count_noexcept() <= 0) return -1.0f;
    float us = -1.0f;
    guarded(1, [&] { us = probe_grid_barrier_us(n_blocks, iters, errors); return 0; });
    return us;
}

// ---- host-only logic -----------------------------------------------------------------------------------------------------------
struct MiniGPT4Vocab { LLMFile f; Tokenizer t; };
struct MiniGPT4Vocab *minigpt4_amd_vocab_load(const char *llm_path) {
    if (!file_exists(llm_path)) return nullptr;
    MiniGPT4Vocab *v = new (std::nothrow) MiniGPT4Vocab();
    if (!v) return nullptr;
    if (v->f.load(llm_path, true)) { delete v; return nullptr; }
    v->t.init(v->f);
    return v;
}
void minigpt4_amd_vocab_free(struct MiniGPT4Vocab *v) { delete v; }
int minigpt4_amd_vocab_size(struct MiniGPT4Vocab *v) { return v ? (int)v->f.n_vocab : 0; }
const char *minigpt4_amd_vocab_piece(struct MiniGPT4Vocab *v, int id, int *len) {
    if (!v || id < 0 || id >= (int)v->f.pieces.size()) return nullptr;
    if (len) *len = (int)v->f.pieces[(size_t)id].size();
    return v->f.pieces[(size_t)id].c_str();
}
int minigpt4_amd_vocab_tokenize(struct MiniGPT4Vocab *v, const char *text, int add_bos, int32_t *out, int cap) {
    if (!v || !text) return -1;
    const std::vector<int> t = v->t.tokenize(text, add_bos != 0);
    for (int i = 0; i < (int)t.size() && i < cap; i++) out[i] = t[(size_t)i];
    return (int)t.size();
}
int minigpt4_amd_inspect_files(const char *vision_path, const char *llm_path, int *n_vision_tensors, int *n_llm_tensors, int64_t *llm_weight_bytes_per_token) {
    if (vision_path) {
        if (!file_exists(vision_path)) return E_PathDoesNotExist;
        VisionFile vf; if (int e = vf.load(vision_path)) return e;
        int n = 0; for (auto &m : vf.models) n += (int)m.second.size();
        if (n_vision_tensors) *n_vision_tensors = n;
    }
    if (llm_path) {
        if (!file_exists(llm_path)) return E_PathDoesNotExist;
        LLMFile lf; if (int e = lf.load(llm_path)) return e;
        if (n_llm_tensors) *n_llm_tensors = (int)lf.tensors.size();
        if (llm_weight_bytes_per_token) { int64_t b = 0; for (auto &t : lf.tensors) b += t.first == "tok_embeddings.weight" ? (int64_t)gt_nbytes(t.second.type, (size_t)t.second.ne[0]) : (int64_t)t.second.nbytes; *llm_weight_bytes_per_token = b; }
    }
    return E_None;
}
int minigpt4_amd_resample_coeffs(int in_size, int out_size, int *ksize, int *first, int *count, int *kk, size_t kk_cap) {
    if (in_size <= 0 || out_size <= 0 || in_size > (1 << 24) || out_size > (1 << 16)) return -1;
    ResampleCoeffs c; precompute_bicubic_8bpc(in_size, out_size, c);
    if (ksize) *ksize = c.ksize;
    if (first) memcpy(first, c.first.data(), (size_t)out_size * 4);
    if (count) memcpy(count, c.count.data(), (size_t)out_size * 4);
    if (kk) { if (kk_cap < c.kk.size()) return -2; memcpy(kk, c.kk.data(), c.kk.size() * 4); }
    return 0;
}
// FNV-1a digest of everything the engine takes from an LLM file: hyper-parameters, vocabulary (pieces + scores) and every tensor (name, type, shape, bytes),
// tensors in name order.  A GGUF file and the GGJT v3 file of the same model must give the same digest.
int minigpt4_amd_llm_file_digest(const char *llm_path, uint64_t *digest, int with_data) {
    if (!llm_path || !digest) return E_LoadLanguageModel;
    if (!file_exists(llm_path)) return E_PathDoesNotExist;
    LLMFile f;
    if (int e = f.load(llm_path)) return e;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) { const uint8_t *b = static_cast<const uint8_t *>(p); for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
    const uint32_t hp[5] = {f.n_vocab, f.n_embd, f.n_head, f.n_layer, f.n_ff()};
    mix(hp, sizeof(hp));
    for (size_t i = 0; i < f.pieces.size(); i++) { const uint32_t n = (uint32_t)f.pieces[i].size(); mix(&n, 4); mix(f.pieces[i].data(), n); mix(&f.scores[i], 4); }
    for (auto &kv : f.tensors) {
        const TensorMeta &t = kv.second;
        mix(kv.first.data(), kv.first.size()); mix(&t.type, 4);
        for (int64_t d : t.ne) mix(&d, 8);
        if (with_data) mix(f.mf.data + t.offset, t.nbytes);
    }
    *digest = h;
    return E_None;
}
int64_t minigpt4_amd_quantize_chunk(int ggml_type, const float *x, void *dst, int64_t n) {
    if (!x || !dst || n <= 0) return 0;
    return (int64_t)quantize_chunk(ggml_type, x, static_cast<uint8_t *>(dst), (size_t)n);
}
int minigpt4_amd_sample_logits(const float *logits, int n_vocab, int seed, float temp, int32_t top_k, float top_p, float tfs_z, float typical_p, int mirostat, float mirostat_tau, float mirostat_eta) {
    if (!logits || n_vocab <= 0) return -1;
    Sampler s; s.seed(seed);
    SampleParams p; p.temp = temp; p.top_k = top_k; p.top_p = top_p; p.tfs_z = tfs_z; p.typical_p = typical_p; p.mirostat = mirostat; p.mirostat_tau = mirostat_tau; p.mirostat_eta = mirostat_eta;
    return s.sample(logits, n_vocab, p);
}

}  // extern "C"
