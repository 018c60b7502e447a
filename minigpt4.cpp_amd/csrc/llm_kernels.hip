// gfx950 kernels for the Vicuna (LLaMA) path: fused-dequant integer-dot mat-vec / mat-mul over repacked weight planes,
// RMSNorm + activation quantisation, RoPE + KV append, causal attention over the fp16 KV cache, argmax, embedding gather.
//
// Arithmetic follows the reference's CPU path (ggml @ llama.cpp master-31cfbb1 behind llama_eval, reference
// minigpt4.cpp:2373/2412): activations are quantised to the weight type's vec_dot_type (Q8_0 / Q8_1 / Q8_K), block dots are
// exact int32 (v_dot4_i32_i8), block results are scaled and accumulated in fp32.  See DESIGN.md "Numerics".
#include "kernels.hpp"
#include "devutil.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <tuple>
#include <type_traits>
#include <vector>
#include <hip/hip_ext.h>

namespace mg4 {

// =====================================================================================================================
// helpers
// =====================================================================================================================
// ---- measurement: kernel symbols and per-dispatch timestamps of the launches (Engine::profile_sites) ----------------------------------------------------------------
// While tracing is on, every launcher of this file notes the symbol it is about to launch, and the launch itself goes through hipExtLaunchKernel with a start / stop
// event pair: the runtime stamps those with the dispatch's own begin / end times -- the interval rocprofv3 --kernel-trace reports -- instead of bracketing the launch
// with marker events (measured +2.0...2.9 us of packet processing per pair, profiles/r02_bench_n1.json vs r02_decode_kernel_stats.csv).
static bool g_kname_on = false;
static char g_kname[192] = "";
struct LaunchProbe { hipEvent_t start, stop; };
static std::vector<LaunchProbe> g_probes;      // one per noted launch since tracing was switched on
static size_t g_probe_next = 0;                // first probe not yet attached to a launch
void kernel_name_tracing(bool on) {
    g_kname_on = on; g_kname[0] = 0;
    if (on) { for (auto &p : g_probes) { HIP_IGNORE(hipEventDestroy(p.start)); HIP_IGNORE(hipEventDestroy(p.stop)); } g_probes.clear(); g_probe_next = 0; }
}
void reset_kernel_name() { g_kname[0] = 0; }
const char *last_kernel_name() { return g_kname; }
size_t launch_probe_count() { return g_probes.size(); }
float launch_probe_us(size_t first, size_t last) {   // sum of the dispatch durations of probes [first, last); call after the stream has been synchronised
    float us = 0.0f;
    for (size_t i = first; i < last && i < g_probes.size(); i++) { float ms = 0.0f; if (hipEventElapsedTime(&ms, g_probes[i].start, g_probes[i].stop) != hipSuccess) return -1.0f; us += ms * 1e3f; }
    return us;
}
static void note_kernel(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void note_kernel(const char *fmt, ...) {
    if (!g_kname_on) return;
    char one[128]; va_list ap; va_start(ap, fmt); vsnprintf(one, sizeof(one), fmt, ap); va_end(ap);
    const size_t have = strlen(g_kname);
    if (have && have + 3 < sizeof(g_kname)) strcat(g_kname, " + ");
    strncat(g_kname, one, sizeof(g_kname) - strlen(g_kname) - 1);
    LaunchProbe p{};
    if (hipEventCreate(&p.start) == hipSuccess && hipEventCreate(&p.stop) == hipSuccess) g_probes.push_back(p);
}
// every kernel launch of this file: plain <<< >>> unless a noted launch is waiting for its probe
template <typename... KA, typename... Args>
static inline void launch_k(void (*k)(KA...), dim3 g, dim3 b, size_t lds, hipStream_t s, Args... args) {
    static_assert(sizeof...(KA) == sizeof...(Args), "kernel argument count");
    if (g_kname_on && g_probe_next < g_probes.size()) {
        LaunchProbe &p = g_probes[g_probe_next++];
        std::tuple<KA...> tup{static_cast<KA>(args)...};
        std::apply([&](auto &...e) { void *ptrs[] = {static_cast<void *>(&e)...}; HIP_IGNORE(hipExtLaunchKernel(reinterpret_cast<const void *>(k), g, b, ptrs, lds, s, p.start, p.stop, 0)); }, tup);
        return;
    }
    k<<<g, b, lds, s>>>(args...);
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, l, s, ...) launch_k(k, g, b, l, s, __VA_ARGS__)

}  // namespace mg4
#include "qtraits.hpp"
#include "row_prep.hpp"
namespace mg4 {

// =====================================================================================================================
// load-time repack: ggml array-of-blocks -> planes.  One thread per unit (16 bytes of the main plane).
// =====================================================================================================================
size_t plan_qweight(int type, int rows, int cols, QWeight &w, uint8_t *base) {
    w = QWeight{};
    w.type = type; w.rows = rows; w.cols = cols;
    const size_t n = (size_t)rows * cols;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { uint8_t *p = base ? base + off : nullptr; off += al(bytes); return p; };
    switch (type) {
    case GT_F32: w.qs = take(n * 4); break;
    case GT_F16: w.qs = take(n * 2); break;
    case GT_Q4_0: w.qs = take(n / 32 * 16); w.sc = take(n / 32 * 2); break;
    case GT_Q4_1: w.qs = take(n / 32 * 16); w.sc = take(n / 32 * 4); break;
    case GT_Q5_0: w.qs = take(n / 32 * 16); w.qh = take(n / 32 * 4); w.sc = take(n / 32 * 2); break;
    case GT_Q5_1: w.qs = take(n / 32 * 16); w.qh = take(n / 32 * 4); w.sc = take(n / 32 * 4); break;
    case GT_Q8_0: w.qs = take(n / 32 * 32); w.sc = take(n / 32 * 2); break;
    case GT_Q2_K: w.qs = take(n / 32 * 8); w.sc = take(n / 32 * 2); w.d = take(n / 256 * 4); break;   // unit = 32 consecutive weights = two 16-weight sub-blocks: 2-bit planes, {scale | min << 4} x 2, {d, dmin} per super-block
    case GT_Q4_K: w.qs = take(n / 256 * 128); w.sc = take(n / 256 * 16); break;
    case GT_Q5_K: w.qs = take(n / 256 * 128); w.qh = take(n / 256 * 32); w.sc = take(n / 256 * 16); break;
    case GT_Q6_K: w.qs = take(n / 256 * 128); w.qh = take(n / 256 * 64); w.sc = take(n / 256 * 16); w.d = take(n / 256 * 2); break;
    default: return 0;
    }
    w.bytes = gt_nbytes(type, n);
    return off;
}
bool qweight_supported(int type) {
    switch (type) { case GT_F32: case GT_F16: case GT_Q4_0: case GT_Q4_1: case GT_Q5_0: case GT_Q5_1: case GT_Q8_0: case GT_Q2_K: case GT_Q4_K: case GT_Q5_K: case GT_Q6_K: return true; default: return false; }
}

// high-bit transposition for 5-bit types: element e of 32 (lo: e<16 -> dword k=e/4, byte i=e%4, slot w=k; hi: e>=16 -> w=4+k)
__device__ __forceinline__ unsigned pack_hb1(const unsigned char hb_lo[16], const unsigned char hb_hi[16]) {
    unsigned P = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) { const int k = e >> 2, i = e & 3; P |= (unsigned)(hb_lo[e] & 1) << (8 * i + k); P |= (unsigned)(hb_hi[e] & 1) << (8 * i + 4 + k); }
    return P;
}

__global__ void k_repack(const uint8_t *__restrict__ raw, QWeight w, size_t n_units) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_units) return;
    uint8_t *qs = const_cast<uint8_t *>(w.qs), *qh = const_cast<uint8_t *>(w.qh), *sc = const_cast<uint8_t *>(w.sc), *dd = const_cast<uint8_t *>(w.d);
    switch (w.type) {
    case GT_Q4_0: { const uint8_t *b = raw + g * 18; sc[g * 2] = b[0]; sc[g * 2 + 1] = b[1]; for (int i = 0; i < 16; i++) qs[g * 16 + i] = b[2 + i]; break; }
    case GT_Q4_1: { const uint8_t *b = raw + g * 20; for (int i = 0; i < 4; i++) sc[g * 4 + i] = b[i]; for (int i = 0; i < 16; i++) qs[g * 16 + i] = b[4 + i]; break; }
    case GT_Q5_0: case GT_Q5_1: {
        const int hdr = w.type == GT_Q5_0 ? 2 : 4; const uint8_t *b = raw + g * (size_t)(hdr + 20);
        for (int i = 0; i < hdr; i++) sc[g * hdr + i] = b[i];
        const unsigned q = (unsigned)b[hdr] | ((unsigned)b[hdr + 1] << 8) | ((unsigned)b[hdr + 2] << 16) | ((unsigned)b[hdr + 3] << 24);
        unsigned char lo[16], hi[16];
        for (int e = 0; e < 16; e++) { lo[e] = (q >> e) & 1; hi[e] = (q >> (16 + e)) & 1; }
        *reinterpret_cast<unsigned *>(qh + g * 4) = pack_hb1(lo, hi);
        for (int i = 0; i < 16; i++) qs[g * 16 + i] = b[hdr + 4 + i];
        break; }
    case GT_Q8_0: { const size_t blk = g >> 1; const int half = (int)(g & 1); const uint8_t *b = raw + blk * 34;
        if (!half) { sc[blk * 2] = b[0]; sc[blk * 2 + 1] = b[1]; }
        for (int i = 0; i < 16; i++) qs[g * 16 + i] = b[2 + half * 16 + i];
        break; }
    case GT_Q2_K: {   // block_q2_K = scales[16] | qs[64] | d | dmin; element 128 n + 32 j + l = (qs[32 n + l] >> 2 j) & 3; unit i of a super-block = elements 32 i .. 32 i + 31
        const size_t sb = g >> 3; const int i = (int)(g & 7), n = i >> 2, j = i & 3; const uint8_t *b = raw + sb * 84;
        if (i == 0) for (int k = 0; k < 4; k++) dd[sb * 4 + k] = b[80 + k];
        unsigned P0 = 0, P1 = 0;   // weight e (0..15) of a half at bits 8 (e & 3) + 2 (e >> 2): (P >> 2 k) & 0x03030303 = the four weights of dword k
        for (int e = 0; e < 16; e++) { const int k = e >> 2, c = e & 3;
            P0 |= (((unsigned)b[16 + 32 * n + e] >> (2 * j)) & 3u) << (8 * c + 2 * k); P1 |= (((unsigned)b[16 + 32 * n + 16 + e] >> (2 * j)) & 3u) << (8 * c + 2 * k); }
        reinterpret_cast<unsigned *>(qs + g * 8)[0] = P0; reinterpret_cast<unsigned *>(qs + g * 8)[1] = P1;
        sc[g * 2] = b[2 * i]; sc[g * 2 + 1] = b[2 * i + 1];
        break; }
    case GT_Q4_K: { const size_t sb = g >> 3; const int u = (int)(g & 7); const uint8_t *b = raw + sb * 144;
        if (u == 0) for (int i = 0; i < 16; i++) sc[sb * 16 + i] = b[i];
        for (int i = 0; i < 16; i++) qs[g * 16 + i] = b[16 + u * 16 + i];
        break; }
    case GT_Q5_K: { const size_t sb = g >> 3; const int u = (int)(g & 7), j = u >> 1, h = u & 1; const uint8_t *b = raw + sb * 176;
        if (u == 0) for (int i = 0; i < 16; i++) sc[sb * 16 + i] = b[i];
        unsigned char lo[16], hi[16];
        for (int e = 0; e < 16; e++) { const unsigned char v = b[16 + 16 * h + e]; lo[e] = (v >> (2 * j)) & 1; hi[e] = (v >> (2 * j + 1)) & 1; }
        *reinterpret_cast<unsigned *>(qh + g * 4) = pack_hb1(lo, hi);
        for (int i = 0; i < 16; i++) qs[g * 16 + i] = b[48 + u * 16 + i];
        break; }
    case GT_Q6_K: { const size_t sb = g >> 3; const int u = (int)(g & 7), n = u >> 2, c = (u >> 1) & 1, h = u & 1; const uint8_t *b = raw + sb * 210;
        if (u == 0) { dd[sb * 2] = b[208]; dd[sb * 2 + 1] = b[209]; }
        unsigned Plo = 0, Phi = 0;
        for (int e = 0; e < 16; e++) { const unsigned v = b[128 + 32 * n + 16 * h + e]; const int k = e >> 2, i = e & 3;
            Plo |= ((v >> (2 * c)) & 3u) << (8 * i + 2 * k); Phi |= ((v >> (4 + 2 * c)) & 3u) << (8 * i + 2 * k); }
        reinterpret_cast<unsigned *>(qh + g * 8)[0] = Plo; reinterpret_cast<unsigned *>(qh + g * 8)[1] = Phi;
        sc[g * 2] = b[192 + 8 * n + 2 * c + h]; sc[g * 2 + 1] = b[192 + 8 * n + 4 + 2 * c + h];
        for (int i = 0; i < 16; i++) qs[g * 16 + i] = b[u * 16 + i];
        break; }
    case GT_F16: case GT_F32: { for (int i = 0; i < 16; i++) qs[g * 16 + i] = raw[g * 16 + i]; break; }
    default: break;
    }
}
void launch_repack(const uint8_t *raw, const QWeight &w, hipStream_t s) {
    const size_t n = (size_t)w.rows * w.cols;
    size_t units;
    switch (w.type) { case GT_F32: units = n / 4; break; case GT_F16: units = n / 8; break; case GT_Q8_0: units = n / 16; break; default: units = n / 32; }
    const int bs = 256;
    hipLaunchKernelGGL(k_repack, dim3((unsigned)((units + bs - 1) / bs)), dim3(bs), 0, s, raw, w, units);
}


// =====================================================================================================================
// y[t][r] = W[r] . act[t] (+ residual).  One wave owns R consecutive rows; its 64 lanes stride over the row's units
// (16-byte coalesced loads, 1 KiB per wave-instruction); each lane keeps the activation unit in registers and reuses it
// for the R rows and TN tokens.  Wave-level xor-shuffle reduction at the end; no LDS.
// =====================================================================================================================
template <int T, int R, int TN>
__global__ __launch_bounds__(256) void k_mul_mat(const QWeight W, const ActQ A, const int N, float *y, const int ldy, const float *residual) {
    using X = Tr<T>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * 4 + wave) * R;
    const int t0 = blockIdx.y * TN;
    if (row0 >= W.rows) return;          // wave-uniform
    const int K = W.cols, U = K / X::EPU;
    float acc[R][TN];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int t = 0; t < TN; t++) acc[r][t] = 0.0f;
    int rows_i[R];
#pragma unroll
    for (int r = 0; r < R; r++) rows_i[r] = min(row0 + r, W.rows - 1);
    for (int u0 = 0; u0 < U; u0 += 64) {
        const int u = u0 + lane;
        const bool ok = u < U;
        const int uc = ok ? u : 0;       // out-of-range lanes fetch unit 0 (valid address), their result is discarded
        typename X::AU a[TN];
#pragma unroll
        for (int t = 0; t < TN; t++) X::loada(A, min(t0 + t, N - 1), K, uc, a[t]);
        typename X::WU w[R];
#pragma unroll
        for (int r = 0; r < R; r++) X::loadw(W, (size_t)rows_i[r] * U, uc, w[r]);
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int t = 0; t < TN; t++) { float c = acc[r][t]; X::dot(w[r], a[t], c); acc[r][t] = ok ? c : acc[r][t]; }
    }
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int t = 0; t < TN; t++) {
            const float v = wave_sum(acc[r][t]);
            if (lane == 0 && row0 + r < W.rows && t0 + t < N) {
                const size_t o = (size_t)(t0 + t) * ldy + row0 + r;
                y[o] = residual ? v + residual[o] : v;
            }
        }
}

template <int T>
static void launch_mul_mat_t(const QWeight &W, const ActQ &A, int N, float *y, int ldy, const float *residual, hipStream_t s) {
    note_kernel("k_mul_mat<%d, 2, %d>", T, N == 1 ? 1 : 4);
    if (N == 1) {
        constexpr int R = 2;
        dim3 grid((unsigned)((W.rows + 4 * R - 1) / (4 * R)), 1);
        hipLaunchKernelGGL((k_mul_mat<T, R, 1>), grid, dim3(256), 0, s, W, A, N, y, ldy, residual);
    } else {
        constexpr int R = 2, TN = 4;
        dim3 grid((unsigned)((W.rows + 4 * R - 1) / (4 * R)), (unsigned)((N + TN - 1) / TN));
        hipLaunchKernelGGL((k_mul_mat<T, R, TN>), grid, dim3(256), 0, s, W, A, N, y, ldy, residual);
    }
}
// =====================================================================================================================
// What is instantiated.  A lane of a decode mat-vec owns NU units of a row (u = lane + 64 i), and every form of the kernel family is built for the unit counts stated
// here and nowhere else: the launchers dispatch on these lists (mv_for_units), and the predicates the engine asks before it fuses a row preparation into a launch are
// computed from them (below), so a shape a predicate accepts is a shape the launcher has.
// =====================================================================================================================
enum EpiKind : int { EPI_STORE = 0, EPI_SILU_PAIR = 1, EPI_REF = 2 };   // EPI_REF (MINIGPT4_PARITY): store, every fp32 accumulation in the CPU oracle's order (ref_chain; the rms sum = the oracle's value)
#ifndef MG4_R_NU3
#define MG4_R_NU3 1
#endif
#ifndef MG4_R_NU2
#define MG4_R_NU2 1
#endif
template <int... NU> struct UnitList {};
using Units1to7 = UnitList<1, 2, 3, 4, 5, 6, 7>;
using Units1to3 = UnitList<1, 2, 3>;
template <int T> constexpr bool tr_is_kquant() { return T == GT_Q4_K || T == GT_Q5_K || T == GT_Q6_K; }
template <int T> constexpr bool tr_is_q32() { return T == GT_Q4_0 || T == GT_Q4_1 || T == GT_Q5_0 || T == GT_Q5_1; }
template <int T> constexpr bool tr_is_narrow() { return T == GT_Q8_0 || T == GT_F16; }   // 16-byte units of 16 / 8 weights: more units per row than the 32-weight types
// k_matvec_v2<T, NU, R, PRO, EPI>.  Q8_0 / F16: only a few unit counts, a row takes the smallest one that covers it (the surplus units are masked like any ragged
// tail) -- Q8_0: K <= 1024 | 4096 | 5120 | 11264; F16: K <= 512 | 1024 | 4096 | 5120.  Pair epilogue (w1|w3): K <= 6144.  EPI_REF: the k-quants of the headline files
// (other types: k_mul_mat_ref_row).
template <int T, int EPI> constexpr auto mv_units() {
    if constexpr (T == GT_Q8_0) return std::conditional_t<EPI == EPI_STORE, UnitList<1, 4, 5, 11>, UnitList<>>{};
    else if constexpr (T == GT_F16) return std::conditional_t<EPI == EPI_STORE, UnitList<1, 2, 8, 10>, UnitList<>>{};
    else if constexpr (tr_is_kquant<T>()) return std::conditional_t<EPI == EPI_SILU_PAIR, Units1to3, Units1to7>{};
    else if constexpr (tr_is_q32<T>()) return std::conditional_t<EPI == EPI_SILU_PAIR, Units1to3, std::conditional_t<EPI == EPI_STORE, Units1to7, UnitList<>>>{};
    else return UnitList<>{};
}
template <int T, int NU, int EPI> constexpr int mv_rows_per_group() {   // R: rows a wave has in flight per stage
    if (EPI == EPI_SILU_PAIR) return 2;
    if (EPI == EPI_REF) return 1;
    if (NU == 1) return 2;
    return tr_is_narrow<T>() ? 1 : NU == 2 ? MG4_R_NU2 : NU == 3 ? MG4_R_NU3 : 1;
}
using MixUnits = UnitList<1, 2, 3, 4>;          // k_matvec_mix<T1, T2, NU, ..>
// k_matvec_tn<T, NU, TN, PRO> (TN = 2..4 rows): every unit count without a preparation, K <= 6144 of Q4_0 and the k-quants with one; k_matvec_tn_mix: K <= 6144
template <int T> constexpr auto mv_tn_units() { return std::conditional_t<tr_is_kquant<T>() || tr_is_q32<T>(), Units1to7, UnitList<>>{}; }
template <int T> constexpr auto mv_tn_pro_units() { return std::conditional_t<T == GT_Q4_0 || tr_is_kquant<T>(), Units1to3, UnitList<>>{}; }
using TnMixUnits = Units1to3;
using RefRowUnits = UnitList<1, 2, 3, 4, 6, 7>;  // k_mul_mat_ref_row / k_mul_mat_ref_rows (the 7B / 13B widths)

template <int... NU> constexpr bool units_have(UnitList<NU...>, int nu) { return ((nu == NU) || ...); }
template <int... NU> constexpr int units_max(UnitList<NU...>) { int m = 0; ((m = NU > m ? NU : m), ...); return m; }
// f(integral_constant<NU>) for the list's entry that equals nu (COVER: the first that covers it); false: no such entry, nothing was called
template <bool COVER = false, int... NU, class F> static bool mv_for_units(UnitList<NU...>, int nu, F &&f) {
    return (((COVER ? nu <= NU : nu == NU) ? (f(std::integral_constant<int, NU>{}), true) : false) || ...);
}
template <class F> static void mv_for_rows(int N, F &&f) {   // TN of N = 1..4 rows: the kernels are vector-issue bound, an unused row costs its share
    if (N <= 2) f(std::integral_constant<int, 2>{}); else if (N == 3) f(std::integral_constant<int, 3>{}); else f(std::integral_constant<int, 4>{});
}
// f(integral_constant<type>) -> bool for a repacked weight type; false: no such type
template <class F> static bool for_weight_type(int type, F &&f) {
    switch (type) {
    case GT_Q4_0: return f(std::integral_constant<int, GT_Q4_0>{});
    case GT_Q4_1: return f(std::integral_constant<int, GT_Q4_1>{});
    case GT_Q5_0: return f(std::integral_constant<int, GT_Q5_0>{});
    case GT_Q5_1: return f(std::integral_constant<int, GT_Q5_1>{});
    case GT_Q8_0: return f(std::integral_constant<int, GT_Q8_0>{});
    case GT_Q2_K: return f(std::integral_constant<int, GT_Q2_K>{});
    case GT_Q4_K: return f(std::integral_constant<int, GT_Q4_K>{});
    case GT_Q5_K: return f(std::integral_constant<int, GT_Q5_K>{});
    case GT_Q6_K: return f(std::integral_constant<int, GT_Q6_K>{});
    case GT_F16: return f(std::integral_constant<int, GT_F16>{});
    case GT_F32: return f(std::integral_constant<int, GT_F32>{});
    default: return false;
    }
}
// the two-type launches: wq|wk + wv of llama.cpp's "more bits" k-quant mixes
template <class F> static bool for_mixed_types(int t1, int t2, F &&f) {
    if (t1 == GT_Q5_K && t2 == GT_Q6_K) return f(std::integral_constant<int, GT_Q5_K>{}, std::integral_constant<int, GT_Q6_K>{});
    if (t1 == GT_Q4_K && t2 == GT_Q6_K) return f(std::integral_constant<int, GT_Q4_K>{}, std::integral_constant<int, GT_Q6_K>{});
    return false;
}
// Largest K of a unit list for a type, 0: none.  A row is a whole number of the type's blocks (F16: of 16-byte units).
template <class L> static bool mv_covers(L list, int type, int K) {
    const int epu = type == GT_F16 ? 8 : type == GT_Q8_0 ? 16 : 32, block = type == GT_F16 ? 8 : gt_block(type);
    return K > 0 && K % block == 0 && K <= units_max(list) * 64 * epu;
}
bool matvec_prologue_supported(int type, int cols) { return for_weight_type(type, [&](auto t) { return mv_covers(mv_units<decltype(t)::value, EPI_STORE>(), type, cols); }); }
bool matvec_silu_pair_supported(int type, int cols) { return for_weight_type(type, [&](auto t) { return mv_covers(mv_units<decltype(t)::value, EPI_SILU_PAIR>(), type, cols); }); }
bool matvec_rows_prologue_ok(int type, int K) { return for_weight_type(type, [&](auto t) { return mv_covers(mv_tn_pro_units<decltype(t)::value>(), type, K); }); }

// =====================================================================================================================
// MINIGPT4_PARITY=1 -- the oracle's fp32 ORDER (oracle/refcpu.c vec_dot_*: one sequential chain of fma's per output, block after block).  One wave per
// (row, token): the lanes split the row's units exactly like k_mul_mat and use the same unit traits (same loads, same integer dot products), but the integer parts are
// first combined per ggml block (8 units per k-quant super-block, 2 per Q8_0 block: exact), and the per-block fp32 terms are then added by every lane in block order.
// The fast kernels differ from this one only in the order of those additions; this one is bit-identical to the CPU oracle.  F16 / F32: one fma per ELEMENT in
// element order (ggml_vec_dot_f16 restated as a scalar loop), unit after unit.
// =====================================================================================================================
template <int T> __device__ __forceinline__ float ref_chunk(const typename Tr<T>::WU &w, const typename Tr<T>::AU &a, const bool ok, const int n_here, float acc);   // below
template <int T>
__global__ __launch_bounds__(256) void k_mul_mat_ref(const QWeight W, const ActQ A, const int N, float *y, const int ldy, const float *residual) {
    using X = Tr<T>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave, t = blockIdx.y;
    if (row >= W.rows || t >= N) return;          // wave-uniform
    const int K = W.cols, U = K / X::EPU;
    float acc = 0.0f;
    for (int u0 = 0; u0 < U; u0 += 64) {
        const int u = u0 + lane;
        const bool ok = u < U;
        const int uc = ok ? u : 0;
        const int n_here = min(64, U - u0);
        typename X::AU a; X::loada(A, t, K, uc, a);
        typename X::WU w; X::loadw(W, (size_t)row * U, uc, w);
        if constexpr (T == GT_F16 || T == GT_F32) {
            for (int g = 0; g < n_here; g++) { float c = acc; X::dot(w, a, c); acc = __shfl(c, g); }   // unit g continues the chain where unit g - 1 left it
        } else {
            acc = ref_chunk<T>(w, a, ok, n_here, acc);
        }
    }
    if (lane == 0) { const size_t o = (size_t)t * ldy + row; y[o] = residual ? acc + residual[o] : acc; }
}
// One chunk of <= 64 units (n_here of them; lane = unit) of one output in the oracle's order: the running value `acc` (wave-uniform) comes in, the value after the chunk's
// last block goes out.
template <int T>
__device__ __forceinline__ float ref_chunk(const typename Tr<T>::WU &w, const typename Tr<T>::AU &a, const bool ok, const int n_here, float acc) {
    using X = Tr<T>;
    int i0, i1; X::ints(w, a, i0, i1);
    if (!ok) { i0 = 0; i1 = 0; }
    // the block's integer parts over its GROUP lanes on the DPP crossbar (exact integer sums: any combining order gives the same value; __shfl_xor is an LDS permute)
    if (X::GROUP >= 2) { i0 += dpp_i<0xB1>(i0); i1 += dpp_i<0xB1>(i1); }
    if (X::GROUP >= 4) { i0 += dpp_i<0x4E>(i0); i1 += dpp_i<0x4E>(i1); }
    if (X::GROUP >= 8) { i0 += dpp_i<0x141>(i0); i1 += dpp_i<0x141>(i1); }
    static_assert(X::GROUP <= 8, "one DPP row half per ggml block");
    float f0, v0, f1, v1; X::terms(w, a, i0, i1, f0, v0, f1, v1);
    if constexpr (X::GROUP == 8) {
        // k-quants: the chain walks the 8-lane groups of this register in place.  At step g every lane takes the running value of the lane 8 below it (row_shr:8:
        // the lower half of its 16-lane row) or, where a row begins, of the previous row's last lane (row_bcast:15), and adds ITS block's terms: after step g the
        // lanes of group g hold the oracle's running sum, the other lanes hold values nobody reads.  3 instructions per block instead of 4 v_readlane + 2 fma.
        const int ng = n_here / 8;
        float run = acc;
#pragma unroll
        for (int g = 0; g < 8; g++) {
            if (g < ng) {
                float t = g == 0 ? acc : ((g & 1) ? dpp_f<0x118>(run) : dpp_f<0x142>(run));
                t = fmaf(f0, v0, t);
                if (X::TERMS == 2) t = fmaf(f1, v1, t);
                run = t;
            }
        }
        acc = readlane_f(run, 8 * (ng - 1));
    } else {
        for (int g = 0; g < n_here; g += X::GROUP) {   // g is wave-uniform: v_readlane (the generic __shfl is an LDS permute, ~100 dependent cycles per block term)
            acc = fmaf(readlane_f(f0, g), readlane_f(v0, g), acc);
            if (X::TERMS == 2) acc = fmaf(readlane_f(f1, g), readlane_f(v1, g), acc);
        }
    }
    return acc;
}
// One output from the lanes' NU registers of units (u = lane + 64 i): chunk after chunk.  Returns the wave-uniform result.
template <int T, int NU>
__device__ __forceinline__ float ref_chain(const typename Tr<T>::WU (&w)[NU], const typename Tr<T>::AU (&a)[NU], const bool (&ok)[NU], const int U) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < NU; i++) {
        const int n_here = min(64, U - 64 * i);
        if (n_here <= 0) break;
        acc = ref_chunk<T>(w[i], a[i], ok[i], n_here, acc);
    }
    return acc;
}
// The same chain for ONE activation row (decode) over up to three matrices of one type and K in one launch: every lane's NU units (u = lane + 64 i, as in k_matvec_v2) are
// requested before the first block is added, so a wave pays one memory round trip instead of one per 64 units (the generic kernel above: 3 ... 7 dependent round trips per
// row, 5.5 ms per 13B token in parity mode).  The per-block terms are added in the same order: chunk after chunk, block after block -- bit-identical to k_mul_mat_ref.
struct RefSet { QWeight w[3]; float *y[3]; const float *res[3]; int n; };
template <int T, int NU>
__global__ __launch_bounds__(256) void k_mul_mat_ref_row(const RefSet S, const ActQ A) {
    using X = Tr<T>;
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.y;
    const QWeight &W = S.w[m];
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), n_waves = (int)gridDim.x * 4;
    const int K = W.cols, U = K / X::EPU, rows = W.rows;
    if (wave >= rows) return;                     // wave-uniform
    typename X::AU a[NU]; bool ok[NU]; int uc[NU];
#pragma unroll
    for (int i = 0; i < NU; i++) { const int u = lane + 64 * i; ok[i] = u < U; uc[i] = ok[i] ? u : 0; X::loada(A, 0, K, uc[i], a[i]); }
    struct Row { typename X::WU w[NU]; };
    auto fetch = [&](int row, Row &Rw) {           // clamped instead of branching: every load of the pipeline is unconditional (counted waits)
        const int r = min(row, rows - 1);
#pragma unroll
        for (int i = 0; i < NU; i++) X::loadw(W, (size_t)r * U, uc[i], Rw.w[i]);
    };
    auto chain = [&](int row, const Row &Rw) {     // the oracle's order: chunk after chunk, block after block
        const float acc = ref_chain<T, NU>(Rw.w, a, ok, U);
        if (lane == 0) { const float *r = S.res[m]; S.y[m][row] = r ? acc + r[row] : acc; }
    };
    Row cur, nxt;                                  // two statically named stages, as in matvec_run: the next row is in flight while this one is chained
    fetch(wave, cur);
    for (int row = wave; row < rows;) {
        fetch(row + n_waves, nxt);
        __builtin_amdgcn_sched_barrier(0);
        chain(row, cur);
        __builtin_amdgcn_sched_barrier(0);
        row += n_waves;
        if (row >= rows) break;
        fetch(row + n_waves, cur);
        __builtin_amdgcn_sched_barrier(0);
        chain(row, nxt);
        __builtin_amdgcn_sched_barrier(0);
        row += n_waves;
    }
}
template <int T> static bool launch_mul_mat_ref_row_t(const RefSet &S, const ActQ &A, const LaunchTuning &tune, hipStream_t s) {
    const int U = S.w[0].cols / Tr<T>::EPU, nu = (U + 63) / 64;
    // persistent waves: ~16 per CU over the whole set, each walking rows wave, wave + n_waves, ...
    const int blocks = std::max(1, std::min((S.w[0].rows + 3) / 4, tune.cus * 4 / S.n));
    const dim3 grid((unsigned)blocks, (unsigned)S.n);
    note_kernel("k_mul_mat_ref_row<%d, %d>", T, nu);
    return mv_for_units(RefRowUnits{}, nu, [&](auto n) { hipLaunchKernelGGL((k_mul_mat_ref_row<T, decltype(n)::value>), grid, dim3(256), 0, s, S, A); });
}
// One activation row against 1..3 equally shaped matrices of one type (parity mode's decode step); false -> shape outside this kernel, use launch_mul_mat_ref per matrix
bool launch_mul_mat_ref_set(const QWeight *const *W, float *const *y, const float *const *res, int n, const ActQ &A, const LaunchTuning &tune, hipStream_t s) {
    if (n < 1 || n > 3) return false;
    RefSet S{}; S.n = n;
    for (int i = 0; i < n; i++) { if (W[i]->type != W[0]->type || W[i]->rows != W[0]->rows || W[i]->cols != W[0]->cols) return false; S.w[i] = *W[i]; S.y[i] = y[i]; S.res[i] = res ? res[i] : nullptr; }
    return for_weight_type(W[0]->type, [&](auto t) {   // (Q8_0 / Q2_K / F16 / F32 rows have other unit widths: the generic kernel serves them)
        constexpr int T = decltype(t)::value;
        if constexpr (tr_is_q32<T>() || tr_is_kquant<T>()) return launch_mul_mat_ref_row_t<T>(S, A, tune, s); else return false;
    });
}
// Prompt rows in parity mode: one wave per WEIGHT row (persistent over rows wave, wave + n_waves, ...), the row's units in registers for all N activation rows -- the
// generic kernel above re-reads the weights once per (output, activation row).  The chain per (row, activation row) is ref_chain's: bit-identical to k_mul_mat_ref.
template <int T, int NU>
__global__ __launch_bounds__(256) void k_mul_mat_ref_rows(const QWeight W, const ActQ A, const int N, float *y, const int ldy, const float *residual) {
    using X = Tr<T>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), n_waves = (int)gridDim.x * 4;
    const int K = W.cols, U = K / X::EPU, rows = W.rows;
    bool ok[NU]; int uc[NU];
#pragma unroll
    for (int i = 0; i < NU; i++) { const int u = lane + 64 * i; ok[i] = u < U; uc[i] = ok[i] ? u : 0; }
    for (int row = wave; row < rows; row += n_waves) {
        typename X::WU w[NU];
#pragma unroll
        for (int i = 0; i < NU; i++) X::loadw(W, (size_t)row * U, uc[i], w[i]);
        typename X::AU a0[NU], a1[NU];              // two statically named stages: the next activation row is in flight while this one is chained
#pragma unroll
        for (int i = 0; i < NU; i++) X::loada(A, 0, K, uc[i], a0[i]);
        for (int t = 0; t < N;) {
#pragma unroll
            for (int i = 0; i < NU; i++) X::loada(A, min(t + 1, N - 1), K, uc[i], a1[i]);
            __builtin_amdgcn_sched_barrier(0);
            { const float acc = ref_chain<T, NU>(w, a0, ok, U); if (lane == 0) { const size_t o = (size_t)t * ldy + row; y[o] = residual ? acc + residual[o] : acc; } }
            __builtin_amdgcn_sched_barrier(0);
            if (++t >= N) break;
#pragma unroll
            for (int i = 0; i < NU; i++) X::loada(A, min(t + 1, N - 1), K, uc[i], a0[i]);
            __builtin_amdgcn_sched_barrier(0);
            { const float acc = ref_chain<T, NU>(w, a1, ok, U); if (lane == 0) { const size_t o = (size_t)t * ldy + row; y[o] = residual ? acc + residual[o] : acc; } }
            __builtin_amdgcn_sched_barrier(0);
            ++t;
        }
    }
}
template <int T> static bool launch_mul_mat_ref_rows_t(const QWeight &W, const ActQ &A, int N, float *y, int ldy, const float *residual, const LaunchTuning &tune, hipStream_t s) {
    const int U = W.cols / Tr<T>::EPU, nu = (U + 63) / 64;
    const dim3 grid((unsigned)std::max(1, std::min((W.rows + 3) / 4, tune.cus * 4)));
    note_kernel("k_mul_mat_ref_rows<%d, %d>", T, nu);
    return mv_for_units(RefRowUnits{}, nu, [&](auto n) { hipLaunchKernelGGL((k_mul_mat_ref_rows<T, decltype(n)::value>), grid, dim3(256), 0, s, W, A, N, y, ldy, residual); });
}
template <int T> static void launch_mul_mat_ref_t(const QWeight &W, const ActQ &A, int N, float *y, int ldy, const float *residual, hipStream_t s) {
    note_kernel("k_mul_mat_ref<%d>", T);
    hipLaunchKernelGGL((k_mul_mat_ref<T>), dim3((unsigned)((W.rows + 3) / 4), (unsigned)N), dim3(256), 0, s, W, A, N, y, ldy, residual);
}
void launch_mul_mat_ref(const QWeight &W, const ActQ &A, int N, float *y, int ldy, const float *residual, const LaunchTuning &tune, hipStream_t s) {
    // prompt rows: the weight row stays in registers for all N activation rows (k-quants; the other types and unit counts take the generic kernel)
    if (N > 1 && for_weight_type(W.type, [&](auto t) {
            constexpr int T = decltype(t)::value;
            if constexpr (tr_is_kquant<T>()) return launch_mul_mat_ref_rows_t<T>(W, A, N, y, ldy, residual, tune, s); else return false; })) return;
    if (!for_weight_type(W.type, [&](auto t) { launch_mul_mat_ref_t<decltype(t)::value>(W, A, N, y, ldy, residual, s); return true; }))
        throw HipError{hipErrorInvalidValue, "unsupported weight type", __FILE__, __LINE__};
}

// =====================================================================================================================
// Decode mat-vec, v2: persistent waves.  The launch covers up to 3 matrices of one type and one K (wq|wk|wv, w1|w3) as one
// concatenated row space.  A wave walks row groups g = wave, wave + n_waves, ...; each lane owns NU fixed units of a row
// (u = lane + 64 i), keeps their activation units in registers for the whole kernel, and software-pipelines the weight
// stream: the R x NU x (2-3) loads of the next row group are issued before the current group's dot products (plain global
// loads straight to VGPRs, counted vmcnt waits by the compiler; no LDS -- the weights are read once and not shared).
// =====================================================================================================================
// Activation preparation fused into the mat-vec prologue (decode): every workgroup redundantly prepares the (tiny, L2-resident) activation
// row in LDS -- rms_norm * w | identity | silu(a) * b, then ggml's Q8_K / Q8_0 quantisation -- while its first weight loads are in flight.
struct ProArgs { const float *x; const float *w; Tables tb; };   // RMS: x, norm weight; PLAIN: x; SILU: a = x, b = w

struct MatSet {
    QWeight w0;            // matrix 0; matrix m has every plane shifted by m * dmat bytes
    long long dmat;        // byte distance between consecutive matrices (identical for all planes)
    float *y0; long long dy;            // outputs: y_m = y0 + m * dy
    const float *res0; long long dres;  // optional residual inputs
    int n;                 // matrices in the set
    int rows_each;         // rows of each matrix
};
// The weight-row fetch of a set, shared by the single-row and the multi-row kernel.  Text, not functions: behind a function boundary (also with rows_each passed in,
// or with the selection handed back in a struct) every k_matvec_v2 / k_matvec_tn instantiation schedules its scalar address arithmetic differently.
// MG4_MATSET_ROW: row `row` of the set's concatenated row space (wave-uniform, clamped by the caller) -> which matrix it belongs to (m1, m2), the row inside it (lr), and
// the buffer descriptors of that weight row (B).  The matrix is selected on the operands themselves (a bool -> int conversion would be done on the vector ALU).
// MG4_MATSET_RES: where that row's residual is read, right after the weight loads have been issued.  MG4_MATSET_M_LR: the same mapping where a result is stored.
#define MG4_MATSET_ROW(X, ms, row, rows_each, U, B) \
    const bool m1 = (row) >= (rows_each), m2 = (row) >= 2 * (rows_each); \
    const int lr = (row) - (m2 ? 2 * (rows_each) : (m1 ? (rows_each) : 0)); \
    const long long d = m2 ? 2 * (ms).dmat : (m1 ? (ms).dmat : 0ll); \
    QWeight W = (ms).w0; \
    W.qs += d; W.qh += d; W.sc += d; W.d += d; \
    WBuf B; \
    X::mkb(W, (size_t)lr * (U), B)
#define MG4_MATSET_RES(res_base, res_stride) ((res_base) + (m2 ? 2 * (res_stride) : (m1 ? (res_stride) : 0ll)) + lr)
#define MG4_MATSET_M_LR(row, rows_each) const int m = (row) >= 2 * (rows_each) ? 2 : ((row) >= (rows_each) ? 1 : 0), lr = (row) - m * (rows_each)
// the residual is always loaded (from a valid address: the output when there is none) and dropped when there is none: no load of the pipeline is conditional
__device__ __forceinline__ float load_res(const float *p) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(mkbuf(reinterpret_cast<const uint8_t *>(p)), 0, 0, 0)); }

// Prologue variants run as ONE fat workgroup per CU of 8..12 waves (512..768 threads): the row preparation is repeated per workgroup, so fewer, fatter
// workgroups repeat it less.  The kernel is compiled for the largest size its register budget admits and launched with the size whose
// rows-per-wave division is the most even (see pick_fat_threads).
constexpr int MV_FAT_MIN = 512;
template <int NU> constexpr int mv_fat_max_threads() { return NU <= 4 ? 768 : 512; }

// EPI_SILU_PAIR (w1|w3 of the feed-forward block; ms.n == 2, R == 2): group g = the row pair (w1[g], w3[g]); the wave writes
// h[g] = silu_table(w1[g] . x) * (w3[g] . x) instead of the two dot products.  The table lookup of a group is consumed one group later, so
// that it never stalls the weight stream.
// In-kernel timeline (diagnostic builds only: make EXTRA=-DMG4_TIMELINE OUT=../libminigpt4_tl.so OBJ=build_tl).  Thread 0 of every workgroup of a decode mat-vec
// stamps the 100 MHz constant clock at: 0 entry, 1 first weight tiles requested, 2 activation row ready (prologue done), 3 first row group finished, 4 last row
// group finished, 5 results stored.  The last launch wins; read with minigpt4_amd_timeline after a single-launch micro-benchmark (tools/timeline.py).
#ifdef MG4_TIMELINE
__device__ unsigned long long g_tl[1024 * 8];
#define MG4_TL(i) do { if (threadIdx.x == 0 && blockIdx.x < 1024) g_tl[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
// prologue forms: the row loads have been issued (before the issue barrier and the first weight requests, which stamp 1 follows); an array of its own, read separately
__device__ unsigned long long g_tl_rows[1024];
#define MG4_TL_ROWS() do { if (threadIdx.x == 0 && blockIdx.x < 1024) g_tl_rows[blockIdx.x] = __builtin_amdgcn_s_memrealtime(); } while (0)
// slots 6 / 7: the LATEST end / entry over all waves of the workgroup (the clock only grows, so atomicMax needs no reset between launches)
#define MG4_TL_ALL(i) do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 1024) atomicMax(&g_tl[blockIdx.x * 8 + (i)], (unsigned long long)__builtin_amdgcn_s_memrealtime()); } while (0)
// the prompt attention's own slots (workgroup = blockIdx.x + gridDim.x * blockIdx.y): 0 entry, 1 scores done, 2 softmax done, 3 P.V done, 4 stored
__device__ unsigned long long g_tla[2048 * 8];
#define MG4_TLP(i) do { const unsigned lb_ = blockIdx.x + gridDim.x * blockIdx.y; if (threadIdx.x == 0 && lb_ < 2048) g_tla[lb_ * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define MG4_TLP(i) do {} while (0)
#define MG4_TL(i) do {} while (0)
#define MG4_TL_ROWS() do {} while (0)
#define MG4_TL_ALL(i) do {} while (0)
#endif
// IB (prologue forms): a raw s_barrier (no wait on data) between the row loads and the first weight requests, so that the row loads of ALL waves of the workgroup are ahead
// of any weight request in the CU's vector-memory queue -- without it the row loads of the late waves queue behind the weight tiles of the early ones, and the row-wide
// barriers wait for the slowest wave (row ready 3.6 -> 3.3 us, profiles/r13_matvec_prefetch_depth.log).  Requesting MORE row groups before the preparation (round 2's
// PRIME2, measured again in round 13 as depths 2 / 3) loses: a wave issues in order, so it reaches its row only after the CU has taken all those requests.
// Kernel arguments: a HEAD of plain pointers and ints in front of the structs.  A wave has its kernel arguments fetched by scalar loads from a cold scalar cache
// before it can issue anything; every dependent batch of such loads is a memory round trip in which the wave has nothing in flight.  So (a) what the first vector-memory
// requests need is a head of plain parameters -- with -amdgpu-kernarg-preload-count (csrc/Makefile: PRELOAD) the command processor has those in SGPRs when the wave
// starts, a struct passed by value ends the preloadable sequence -- (b) nothing on that path is a hidden argument (blockDim.x is the explicit nthr), and (c) every field of
// the structs behind the head that the kernel reads is requested in ONE batch (mv_pin_tail: an empty asm statement that consumes the values, so hipcc cannot sink their
// loads behind the row loads or a branch): at entry when nothing is preloaded -- one round trip in all -- or, in a preload build, right after the row loads have been
// issued from the preloaded head, so the batch is in flight with them.  The head's fields shadow their twins in the structs, which the kernels no longer read.
#ifndef MG4_KERNARG_PRELOAD
#define MG4_KERNARG_PRELOAD 0
#endif
constexpr bool MV_PIN_AT_ENTRY = MG4_KERNARG_PRELOAD == 0;
template <int T, int PRO, int EPI>
__device__ __forceinline__ void mv_pin_tail(const MatSet &ms, const ActQ &A, const Tables &tb) {
    asm volatile("" ::"s"(ms.w0.qs), "s"(ms.w0.qh), "s"(ms.w0.sc), "s"(ms.w0.d), "s"(ms.dmat), "s"(ms.y0), "s"(ms.dy), "s"(ms.res0), "s"(ms.dres), "s"(ms.n), "s"(ms.rows_each));
    if (PRO == PRO_SILU || EPI == EPI_SILU_PAIR) asm volatile("" ::"s"(tb.silu));
    if (PRO == PRO_NONE && tr_is_kquant<T>()) asm volatile("" ::"s"(A.q8k), "s"(A.dk), "s"(A.bsk));
}
template <int T, int NU, int R, int PRO, int EPI, bool IB = false>
__device__ __forceinline__ void matvec_run(const MatSet &ms, const ActQ &A, const ProArgs &pa, const int n_groups, const int n_waves, const int wave, const int nthr) {
    static_assert(EPI != EPI_SILU_PAIR || R == 2, "the SiLU pair epilogue works on row pairs");
    static_assert(PRO != PRO_NONE || !IB, "the issue barrier belongs to the prologue forms");
    // groups of this wave: g = g_first, g_first + g_step, ... < g_last
    const int g_first = wave, g_last = n_groups, g_step = n_waves;
    MG4_TL(0); MG4_TL_ALL(7);
    using X = TrMV<T>;
    const int lane = threadIdx.x & 63;
    const int K = ms.w0.cols, U = K / X::EPU, rows_each = ms.rows_each, total_rows = ms.n * rows_each;
    int uc[NU]; bool ok[NU];
#pragma unroll
    for (int i = 0; i < NU; i++) { const int u = lane + 64 * i; ok[i] = u < U; uc[i] = ok[i] ? u : 0; }
    // NOTE: every load of the pipeline is unconditional (indices are clamped instead of branching): a load inside an exec-masked branch
    // makes hipcc's counted s_waitcnt fall back to (near) vmcnt(0), which drains the prefetch -- see DESIGN.md "mat-vec pipeline".
    struct Grp { typename X::WU w[R][NU]; float res[R]; };
    const bool has_res = ms.res0 != nullptr;
    const float *res_base = has_res ? ms.res0 : ms.y0;                     // always a valid address; the value is dropped when there is no residual
    const long long res_stride = has_res ? ms.dres : ms.dy;
    auto fetch = [&](int g, Grp &G) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            // wave-uniform (scalar) row, clamped instead of branching
            const int row = EPI == EPI_SILU_PAIR ? min(g, rows_each - 1) + r * rows_each : min(g * R + r, total_rows - 1);
            MG4_MATSET_ROW(X, ms, row, rows_each, U, B);
#pragma unroll
            for (int i = 0; i < NU; i++) X::loadb(B, uc[i], G.w[r][i]);
            G.res[r] = load_res(MG4_MATSET_RES(res_base, res_stride));
        }
    };
    Grp cur, nxt;
    typename X::AU a[NU];
    if (PRO == PRO_NONE) {
        fetch(g_first, cur);
        MG4_TL(1);
#pragma unroll
        for (int i = 0; i < NU; i++) X::loada(A, 0, K, uc[i], a[i]);
        MG4_TL(2);
    } else {
        // Row preparation in the prologue.  Order matters (vector-memory results return in issue order): the row (and, for SiLU, the table
        // gathers) is requested BEFORE the first weight tiles, so the preparation runs while those tiles are in flight.
        extern __shared__ __attribute__((aligned(16))) unsigned char smem_mv[];
        ActQ L;                                     // LDS image of the quantised row (only the planes this weight type reads are written)
        double *red = reinterpret_cast<double *>(smem_mv);               // [waves] partial sums (dynamic LDS: shared by both halves of k_matvec_mix)
        row_image(L, smem_mv + 128, K);
        L.xh = reinterpret_cast<__half *>(smem_mv + 128);                // F16 weights: the fp16 row takes the place of the two int8 images (2 K bytes)
        L.xf = nullptr;
        constexpr int RND = (NU * 64 * X::EPU / 4 + MV_FAT_MIN - 1) / MV_FAT_MIN;    // K <= NU * 64 * EPU elements, 4 per thread per round, >= MV_FAT_MIN threads
        constexpr int mask = T == GT_F16 ? ACT_F16 : (T == GT_Q4_K || T == GT_Q5_K || T == GT_Q6_K) ? ACT_Q8K : ACT_Q80;
        float4 xv[RND], yv[RND];
        bool in[RND];
#pragma unroll
        for (int r = 0; r < RND; r++) {
            const int i = (r * nthr + (int)threadIdx.x) * 4;
            in[r] = i < K;
            const int ic = in[r] ? i : 0;
            xv[r] = *reinterpret_cast<const float4 *>(pa.x + ic);
            if (PRO != PRO_PLAIN) yv[r] = *reinterpret_cast<const float4 *>(pa.w + ic);
        }
        if (PRO == PRO_SILU) {
#pragma unroll
            for (int r = 0; r < RND; r++) { xv[r].x = tab(pa.tb.silu, xv[r].x); xv[r].y = tab(pa.tb.silu, xv[r].y); xv[r].z = tab(pa.tb.silu, xv[r].z); xv[r].w = tab(pa.tb.silu, xv[r].w); }
        }
        MG4_TL_ROWS();
        if (!MV_PIN_AT_ENTRY) mv_pin_tail<T, PRO, EPI>(ms, A, pa.tb);   // the row loads above needed the preloaded head only; the rest has been on its way meanwhile
        if (IB) {   // orders ISSUE only: nothing is waited for
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        fetch(g_first, cur);
        MG4_TL(1);
        float scale = 1.0f;
        if (PRO == PRO_RMS) {
            double sum = 0.0;
#pragma unroll
            for (int r = 0; r < RND; r++) {
                const float4 v = xv[r];
                double q = 0.0;
                MG4_ROW_SUMSQ4(q, v);
                sum += in[r] ? q : 0.0;
            }
            row_partial(red, sum);
            __syncthreads();
            double tot = 0.0;
            for (int w = 0; w < nthr / 64; w++) tot += red[w];   // row_total's loop as text: called as a function, these kernels (and only these) compile differently
            float mean;
            if (EPI == EPI_REF) MG4_ROW_MEAN_ORACLE(mean, tot, K, pa.x, red); else mean = row_mean(tot, K);
            scale = row_scale(mean);
        }
#pragma unroll
        for (int r = 0; r < RND; r++) {
            const int i = (r * nthr + (int)threadIdx.x) * 4;
            float v[4];
            row_value4<PRO>(v, xv[r], yv[r], scale);
            row_zero_unless(v, in[r]);
            quant_emit4(v, in[r], i, 0, K, L, mask);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NU; i++) X::loada(L, 0, K, uc[i], a[i]);
        MG4_TL(2);
    }
    unsigned short pend_t = 0; float pend_b = 0.0f; int pend_row = -1;          // EPI_SILU_PAIR: the previous group's table lookup, not yet consumed
    auto flush_pending = [&]() { if (pend_row >= 0 && lane == 0) ms.y0[pend_row] = h2f_bits(pend_t) * pend_b; };
    auto consume = [&](int g, const Grp &G) {
        float out[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            if constexpr (EPI == EPI_REF) out[r] = ref_chain<T, NU>(G.w[r], a, ok, U);
            else {
                float acc = 0.0f;
#pragma unroll
                for (int i = 0; i < NU; i++) { float c = acc; X::dot(G.w[r][i], a[i], c); acc = ok[i] ? c : acc; }
                out[r] = wave_sum(acc);
            }
        }
        if (EPI == EPI_SILU_PAIR) {
            flush_pending();
            pend_t = reinterpret_cast<const unsigned short *>(pa.tb.silu)[f2h_bits(out[0])]; pend_b = out[R - 1]; pend_row = g;
        } else {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int row = g * R + r;
                if (lane == 0 && row < total_rows) {
                    MG4_MATSET_M_LR(row, rows_each);
                    const float val = has_res ? out[r] + G.res[r] : out[r];
                    ms.y0[(long long)m * ms.dy + lr] = val;
                }
            }
        }
    };
    // two statically named stages (a `cur = nxt` copy would have to wait for the loads in flight; the requested unroll is refused by the compiler)
    // The sched_barriers keep the next group's loads ahead of the current group's dot products (the scheduler otherwise hoists the arithmetic, and
    // with it the wait for the current tiles, above the loads: one tile in flight instead of two).
    for (int g = g_first; g < g_last;) {
        fetch(g + g_step, nxt);
        __builtin_amdgcn_sched_barrier(0);
        consume(g, cur);
        __builtin_amdgcn_sched_barrier(0);
#ifdef MG4_TIMELINE
        if (g == g_first) MG4_TL(3);
#endif
        g += g_step;
        if (g >= g_last) break;
        fetch(g + g_step, cur);
        __builtin_amdgcn_sched_barrier(0);
        consume(g, nxt);
        __builtin_amdgcn_sched_barrier(0);
        g += g_step;
    }
    MG4_TL(4);
    if (EPI == EPI_SILU_PAIR) flush_pending();
#ifdef MG4_TIMELINE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    MG4_TL(5); MG4_TL_ALL(6);
#endif
}
// Prologue forms.  Head (8 dwords): the row, the norm weight / second factor, K, the workgroup's thread count, the wave's share of the row groups.
template <int T, int NU, int R, int PRO, int EPI, bool IB = false>
__global__ __launch_bounds__(mv_fat_max_threads<NU>()) void k_matvec_v2(const float *x, const float *w, const int K, const int nthr, const int n_groups, const int n_waves,
                                                                        const MatSet ms_, const ActQ A, const Tables tb) {
    static_assert(PRO != PRO_NONE, "the prologue-free form is k_matvec_v2_free");
    MatSet ms = ms_; ms.w0.cols = K;
    ProArgs pa; pa.x = x; pa.w = w; pa.tb = tb;
    if (MV_PIN_AT_ENTRY) mv_pin_tail<T, PRO, EPI>(ms, A, tb);
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (nthr >> 6) + (threadIdx.x >> 6));   // wave-uniform: scalar loop control
    matvec_run<T, NU, R, PRO, EPI, IB>(ms, A, pa, n_groups, n_waves, wave, nthr);
}
// Prologue-free form (256 threads).  Head (14 dwords): matrix 0's planes, the Q8_K plane of the prepared row, K, rows per matrix, the wave's share of the row groups.
template <int T, int NU, int R, int EPI>
__global__ __launch_bounds__(256) void k_matvec_v2_free(const uint8_t *qs, const uint8_t *qh, const uint8_t *sc, const uint8_t *d, int8_t *q8k, const int K, const int rows_each,
                                                        const int n_groups, const int n_waves, const MatSet ms_, const ActQ A_, const Tables tb) {
    MatSet ms = ms_; ms.w0.qs = qs; ms.w0.qh = qh; ms.w0.sc = sc; ms.w0.d = d; ms.w0.cols = K; ms.rows_each = rows_each;
    ActQ A = A_; A.q8k = q8k;
    ProArgs pa{}; pa.tb = tb;
    mv_pin_tail<T, PRO_NONE, EPI>(ms, A, tb);   // the first weight request needs dmat and n from behind the head: one batch, at entry, in either build
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    matvec_run<T, NU, R, PRO_NONE, EPI, false>(ms, A, pa, n_groups, n_waves, wave, 256);
}
// Two weight types in one launch (llama.cpp's k-quant mixes give wv more bits than wq|wk): waves [0, n_waves1) stream set 1, the rest set 2.  Both
// sets share K and the prepared activation row (both types read the Q8_K image); every wave passes the same number of workgroup barriers.
// Head (10 dwords): as the prologue forms', with both sets' shares (a prologue-free launch passes null rows).
template <int T1, int T2, int NU, int PRO, int EPI = EPI_STORE, bool IB = false>
__global__ __launch_bounds__(PRO == PRO_NONE ? 256 : mv_fat_max_threads<NU>()) void k_matvec_mix(const float *x, const float *w, const int K, const int nthr, const int n_groups1,
                                                                                                 const int n_waves1, const int n_groups2, const int n_waves2, const MatSet ms1_,
                                                                                                 const MatSet ms2_, const ActQ A, const Tables tb) {
    MatSet ms1 = ms1_, ms2 = ms2_; ms1.w0.cols = K; ms2.w0.cols = K;
    ProArgs pa; pa.x = x; pa.w = w; pa.tb = tb;
    if (MV_PIN_AT_ENTRY || PRO == PRO_NONE) { mv_pin_tail<T1, PRO, EPI>(ms1, A, tb); mv_pin_tail<T2, PRO, EPI>(ms2, A, tb); }   // in front of the branch: one batch for either side
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (nthr >> 6) + (threadIdx.x >> 6));
    if (wave < n_waves1) matvec_run<T1, NU, 1, PRO, EPI, IB>(ms1, A, pa, n_groups1, n_waves1, wave, nthr);
    else matvec_run<T2, NU, 1, PRO, EPI, IB>(ms2, A, pa, n_groups2, n_waves2, wave - n_waves1, nthr);
}
// Launch geometry (measured on the 13B decode, profiles/r01g_ab_geometry.log): 8 waves per CU everywhere.  More waves lose even where they divide
// the rows more evenly (5120 rows: 2048 waves = 3 | 2 rows per wave, 2560 waves = 2 each, yet 640-thread workgroups are 6 % slower end to
// end than 512-thread ones; 1024-thread ones 5 % slower; 5 / 7 waves per CU for the K = 13824 mat-vec 4 % / 1 % slower than 8).  The fat (prologue) workgroups have
// MV_FAT_MIN threads outside parity mode.
static int pick_waves_per_cu(const LaunchTuning &tune, int max_wpc) { return std::min(tune.mv_waves_per_cu ? tune.mv_waves_per_cu : 8, max_wpc); }
int matvec_prologue_waves(const LaunchTuning &tune) { return tune.cus * (MV_FAT_MIN / 64); }
static size_t mv_prologue_lds(int K) { return 128 + row_image_bytes(K); }   // the per-wave partial sums, then the row
template <int NU> constexpr int mv_max_wpc() { return NU <= 3 ? 16 : NU == 4 ? 12 : 8; }      // register budget of the two-stage pipeline
// The issue-barrier forms are built for the k-quants at NU <= 3 (K <= 6144: every prologue launch of the 7B / 13B decode step) outside parity mode; elsewhere the launch runs
// the plain form.
template <int T, int NU, int EPI> constexpr bool mv_issue_bar_built() { return (T == GT_Q4_K || T == GT_Q5_K || T == GT_Q6_K) && NU <= 3 && EPI != EPI_REF; }
template <int T, int NU, int R, int PRO, int EPI>
static void launch_v2_pro(bool issue_bar, dim3 grid, dim3 block, size_t lds, hipStream_t s, const MatSet &ms, const ActQ &A, const ProArgs &pa, int n_groups, int n_waves) {
    const bool bar = issue_bar && mv_issue_bar_built<T, NU, EPI>();
    note_kernel("k_matvec_v2<%d, %d, %d, %d, %d, %s>", T, NU, R, PRO, EPI, bar ? "true" : "false");
    if constexpr (mv_issue_bar_built<T, NU, EPI>()) {
        if (bar) { hipLaunchKernelGGL((k_matvec_v2<T, NU, R, PRO, EPI, true>), grid, block, lds, s, pa.x, pa.w, ms.w0.cols, (int)block.x, n_groups, n_waves, ms, A, pa.tb); return; }
    }
    hipLaunchKernelGGL((k_matvec_v2<T, NU, R, PRO, EPI>), grid, block, lds, s, pa.x, pa.w, ms.w0.cols, (int)block.x, n_groups, n_waves, ms, A, pa.tb);
}
template <int T, int NU, int R, int EPI>
static void launch_v2_t(const MatSet &ms, const ActQ &A, int pro, const ProArgs &pa, bool issue_bar, const LaunchTuning &tune, hipStream_t s) {
    const int total_rows = ms.n * ms.rows_each;
    const int n_groups = EPI == EPI_SILU_PAIR ? ms.rows_each : (total_rows + R - 1) / R;
    if (pro == PRO_NONE) {
        note_kernel("k_matvec_v2_free<%d, %d, %d, %d>", T, NU, R, (int)EPI);
        // EPI_REF: the block chain is a dependent sequence per wave (DPP move + fma per block): as many waves per SIMD as the registers admit, not the stream-optimal 8 per CU
        int n_waves = std::min(n_groups, tune.cus * (EPI == EPI_REF ? mv_max_wpc<NU>() : pick_waves_per_cu(tune, mv_max_wpc<NU>())));
        n_waves = (n_waves + 3) & ~3;
        hipLaunchKernelGGL((k_matvec_v2_free<T, NU, R, EPI>), dim3((unsigned)(n_waves / 4)), dim3(256), 0, s, ms.w0.qs, ms.w0.qh, ms.w0.sc, ms.w0.d, A.q8k, ms.w0.cols, ms.rows_each,
                           n_groups, n_waves, ms, A, pa.tb);
        return;
    }
    const int LB = EPI == EPI_REF ? mv_fat_max_threads<NU>() : MV_FAT_MIN, WPB = LB / 64;
    const int n_blocks = std::min((n_groups + WPB - 1) / WPB, tune.cus);
    const int n_waves = n_blocks * WPB;
    const dim3 grid((unsigned)n_blocks), block((unsigned)LB);
    const int K = ms.w0.cols;
    const size_t lds = mv_prologue_lds(K);
    if constexpr (EPI == EPI_SILU_PAIR) {   // w1|w3 follow the ffn norm: only that prologue is instantiated for the pair epilogue
        launch_v2_pro<T, NU, R, PRO_RMS, EPI>(issue_bar, grid, block, lds, s, ms, A, pa, n_groups, n_waves);
    } else switch (pro) {
    case PRO_RMS: launch_v2_pro<T, NU, R, PRO_RMS, EPI>(issue_bar, grid, block, lds, s, ms, A, pa, n_groups, n_waves); break;
    case PRO_PLAIN: launch_v2_pro<T, NU, R, PRO_PLAIN, EPI>(issue_bar, grid, block, lds, s, ms, A, pa, n_groups, n_waves); break;
    default: { if constexpr (EPI == EPI_STORE) launch_v2_pro<T, NU, R, PRO_SILU, EPI>(issue_bar, grid, block, lds, s, ms, A, pa, n_groups, n_waves); } break;
    }
}
template <int T>
static bool launch_v2_type(const MatSet &ms, const ActQ &A, int pro, const ProArgs &pa, int epi, bool issue_bar, const LaunchTuning &tune, hipStream_t s) {
    const int nu = (ms.w0.cols / TrMV<T>::EPU + 63) / 64;
    auto launch = [&](auto e) {
        constexpr int EPI = decltype(e)::value;
        return mv_for_units<tr_is_narrow<T>()>(mv_units<T, EPI>(), nu, [&](auto n) {
            constexpr int NU = decltype(n)::value;
            launch_v2_t<T, NU, mv_rows_per_group<T, NU, EPI>(), EPI>(ms, A, pro, pa, issue_bar, tune, s); });
    };
    switch (epi) {
    case EPI_SILU_PAIR: return ms.n == 2 && (pro == PRO_NONE || pro == PRO_RMS) && launch(std::integral_constant<int, EPI_SILU_PAIR>{});
    case EPI_REF: return pro != PRO_SILU && launch(std::integral_constant<int, EPI_REF>{});   // parity mode has no SiLU prologue (the row comes from k_silu_mul_quant)
    default: return launch(std::integral_constant<int, EPI_STORE>{});
    }
}
// copies the timeline stamps of the last decode mat-vec launch (8 x u64 per workgroup); 0 when the library was built without MG4_TIMELINE
int read_attn_timeline(unsigned long long *out, int max_workgroups) {
#ifdef MG4_TIMELINE
    const int n = std::min(max_workgroups, 2048);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tla), (size_t)n * 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
    return n;
#else
    (void)out; (void)max_workgroups; return 0;
#endif
}
int read_matvec_timeline(unsigned long long *out, int max_workgroups) {
#ifdef MG4_TIMELINE
    const int n = std::min(max_workgroups, 1024);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tl), (size_t)n * 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
    return n;
#else
    (void)out; (void)max_workgroups; return 0;
#endif
}

int read_matvec_timeline_rows(unsigned long long *out, int max_workgroups) {   // one stamp per workgroup: the row loads of a prologue launch issued
#ifdef MG4_TIMELINE
    const int n = std::min(max_workgroups, 1024);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tl_rows), (size_t)n * sizeof(unsigned long long)) != hipSuccess) return -1;
    return n;
#else
    (void)out; (void)max_workgroups; return 0;
#endif
}

static bool fill_matset(MatSet &ms, const QWeight *const *W, float *const *y, const float *const *residual, int n) {
    ms = MatSet{};
    ms.n = n; ms.rows_each = W[0]->rows; ms.w0 = *W[0]; ms.y0 = y[0]; ms.res0 = residual ? residual[0] : nullptr;
    if (n > 1) {
        ms.dmat = (long long)(W[1]->qs - W[0]->qs); ms.dy = (long long)(y[1] - y[0]); ms.dres = residual && residual[0] ? (long long)(residual[1] - residual[0]) : 0;
        for (int i = 1; i < n; i++) {
            if (W[i]->type != W[0]->type || W[i]->rows != W[0]->rows || W[i]->cols != W[0]->cols) return false;
            if ((long long)(W[i]->qs - W[0]->qs) != i * ms.dmat || (W[0]->qh && (long long)(W[i]->qh - W[0]->qh) != i * ms.dmat) ||
                (W[0]->sc && (long long)(W[i]->sc - W[0]->sc) != i * ms.dmat) || (W[0]->d && (long long)(W[i]->d - W[0]->d) != i * ms.dmat)) return false;
            if ((long long)(y[i] - y[0]) != i * ms.dy) return false;
            if (residual && residual[0] && (long long)(residual[i] - residual[0]) != i * ms.dres) return false;
        }
    }
    return true;
}
// Two sets in one launch of `total` workgroups of `wpb` waves: how many of them stream set 1, so that the busiest wave of either set finishes earliest
// (cost = rows per wave x bytes per row)
static int mv_split_blocks(int ng1, double bytes1, int ng2, double bytes2, int total, int wpb) {
    const double bpr1 = bytes1 / ng1, bpr2 = bytes2 / ng2;
    int best_b1 = 1; double best_cost = 1e300;
    for (int b1 = 1; b1 < total; b1++) {
        const int w1 = b1 * wpb, w2 = (total - b1) * wpb;
        const double c = std::max((double)((ng1 + w1 - 1) / w1) * bpr1, (double)((ng2 + w2 - 1) / w2) * bpr2);
        if (c < best_cost) { best_cost = c; best_b1 = b1; }
    }
    return best_b1;
}
template <int T1, int T2, int NU, int EPI = EPI_STORE>
static void launch_mix_t(const MatSet &m1, const MatSet &m2, double bytes1, double bytes2, const ActQ &A, int pro, const ProArgs &pa, bool issue_bar, const LaunchTuning &tune, hipStream_t s) {
    const int ng1 = m1.n * m1.rows_each, ng2 = m2.n * m2.rows_each;
    const int threads = pro == PRO_NONE ? 256 : (EPI == EPI_REF ? mv_fat_max_threads<NU>() : MV_FAT_MIN), wpb = threads / 64;
    const int total = pro == PRO_NONE ? tune.cus * (EPI == EPI_REF ? mv_max_wpc<NU>() : pick_waves_per_cu(tune, mv_max_wpc<NU>())) / 4 : tune.cus;
    const int b1 = mv_split_blocks(ng1, bytes1, ng2, bytes2, total, wpb), nw1 = b1 * wpb, nw2 = (total - b1) * wpb;
    constexpr bool BUILT = mv_issue_bar_built<T1, NU, EPI>() && mv_issue_bar_built<T2, NU, EPI>();
    const bool bar = pro != PRO_NONE && issue_bar && BUILT;
    note_kernel("k_matvec_mix<%d, %d, %d, %d, %d, %s>", T1, T2, NU, pro == PRO_NONE ? 0 : 1, (int)EPI, bar ? "true" : "false");
    const dim3 grid((unsigned)total), block((unsigned)threads);
    if (pro == PRO_NONE) { hipLaunchKernelGGL((k_matvec_mix<T1, T2, NU, PRO_NONE, EPI>), grid, block, 0, s, pa.x, pa.w, m1.w0.cols, threads, ng1, nw1, ng2, nw2, m1, m2, A, pa.tb); return; }
    if constexpr (BUILT) {
        if (bar) { hipLaunchKernelGGL((k_matvec_mix<T1, T2, NU, PRO_RMS, EPI, true>), grid, block, mv_prologue_lds(m1.w0.cols), s, pa.x, pa.w, m1.w0.cols, threads, ng1, nw1, ng2, nw2, m1, m2, A, pa.tb); return; }
    }
    hipLaunchKernelGGL((k_matvec_mix<T1, T2, NU, PRO_RMS, EPI>), grid, block, mv_prologue_lds(m1.w0.cols), s, pa.x, pa.w, m1.w0.cols, threads, ng1, nw1, ng2, nw2, m1, m2, A, pa.tb);
}
template <int T1, int T2, int EPI = EPI_STORE>
static bool launch_mix_nu(const MatSet &m1, const MatSet &m2, double b1, double b2, const ActQ &A, int pro, const ProArgs &pa, bool issue_bar, const LaunchTuning &tune, hipStream_t s) {
    return mv_for_units(MixUnits{}, (m1.w0.cols / 32 + 63) / 64, [&](auto n) { launch_mix_t<T1, T2, decltype(n)::value, EPI>(m1, m2, b1, b2, A, pro, pa, issue_bar, tune, s); });
}
// Decode mat-vec over two sets of different k-quant types with the same K (wq|wk + wv of a "more bits" layer) in ONE launch.  pro: PRO_NONE or PRO_RMS.
bool launch_matvec_mixed(const QWeight *const *W1, float *const *y1, int n1, const QWeight *const *W2, float *const *y2, int n2, const ActQ &A, const LaunchTuning &tune, hipStream_t s, int pro,
                         const float *px, const float *pw, int epi, bool issue_bar) {
    if (pro != PRO_NONE && pro != PRO_RMS) return false;
    if (W1[0]->cols != W2[0]->cols || W1[0]->cols % 256) return false;
    MatSet m1, m2;
    if (!fill_matset(m1, W1, y1, nullptr, n1) || !fill_matset(m2, W2, y2, nullptr, n2)) return false;
    ProArgs pa{}; pa.x = px; pa.w = pw;
    double b1 = 0, b2 = 0;
    for (int i = 0; i < n1; i++) b1 += (double)W1[i]->bytes;
    for (int i = 0; i < n2; i++) b2 += (double)W2[i]->bytes;
    return for_mixed_types(W1[0]->type, W2[0]->type, [&](auto t1, auto t2) {
        constexpr int T1 = decltype(t1)::value, T2 = decltype(t2)::value;
        return epi == EPI_REF ? launch_mix_nu<T1, T2, EPI_REF>(m1, m2, b1, b2, A, pro, pa, issue_bar, tune, s) : launch_mix_nu<T1, T2>(m1, m2, b1, b2, A, pro, pa, issue_bar, tune, s); });
}
// Decode (N = 1) mat-vec over 1..3 same-type, same-shape, equally spaced matrices.  Returns false when the set is outside the v2 kernel's range.
bool launch_matvec_set(const QWeight *const *W, float *const *y, const float *const *residual, int n, const ActQ &A, const LaunchTuning &tune, hipStream_t s, int pro, const float *px, const float *pw,
                       const Tables *tb, int epi, bool issue_bar) {
    ProArgs pa{}; pa.x = px; pa.w = pw; if (tb) pa.tb = *tb;
    MatSet ms;
    if (!fill_matset(ms, W, y, residual, n)) return false;
    // false: F32 / Q2_K rows, and rows wider than the type's unit counts (served by k_mul_mat)
    return for_weight_type(W[0]->type, [&](auto t) { return launch_v2_type<decltype(t)::value>(ms, A, pro, pa, epi, issue_bar, tune, s); });
}


// =====================================================================================================================
// Batched decode mat-vec (B conversations, one row each): the same persistent-wave two-stage weight pipeline as k_matvec_v2, for up to TN
// activation rows.  The weights are streamed ONCE; every weight unit is multiplied against the matching activation unit of each row.  The
// quantised activation rows (prepared by k_rms_quant / k_silu_mul_quant) are copied into LDS once per workgroup -- one fat workgroup per CU --
// and read from there inside the loop (registers could hold only K <= 6144 for four rows; LDS traffic is ~1/4 of its bandwidth at HBM speed).
// Per row the arithmetic is exactly the single-row kernel's: the same unit dot products, the same per-lane fma order, the same wave reduction.
// =====================================================================================================================
static size_t mv_tn_lds(int type, int K, int TN) {
    const bool kq = type == GT_Q4_K || type == GT_Q5_K || type == GT_Q6_K;
    const size_t per_row = kq ? (size_t)K + (size_t)(K / 256) * 4 + (size_t)(K / 16) * 2 : (size_t)K + (size_t)(K / 32) * 16;
    return (size_t)TN * per_row + 64;
}
// Are the TN rows' activation fragments register-resident?  512-thread workgroups (two waves per SIMD): 256 registers -> K <= 3 x 64 units at 4 rows, <= 5 x 64 at
// 2 rows; the widest K (NU = 7, K = 13824: w2) runs 256-thread workgroups, one wave per SIMD, 512 registers -> resident at 2 and at 4 rows (4 x 7 x 10 = 280 registers).
template <int NU, int TN> constexpr bool mv_tn_reg() { return NU <= 3 || (TN == 2 && NU <= 5) || NU >= 7; }
template <int NU> constexpr int mv_tn_threads() { return NU >= 7 ? 256 : 512; }   // widest K: one wave per SIMD (up to 512 VGPRs) -- two would spill Q5_K's weight stages; 4 waves x 7 units keep as many bytes in flight as 8 x 3
// PRO = 1 (K <= 3 x 64 units only): the rows are prepared inside the launch -- rms_norm(x_t) * w and the quantisation of k_rms_quant, row by row with the single-row
// prologue's arithmetic (matvec_run), into one LDS image per row -- so a batched decode step needs no standalone preparation launch in front of wq|wk|wv and w1|w3.
static size_t mv_tn_image_bytes(int K) { return (row_image_bytes(K) + 15) & ~(size_t)15; }
extern __shared__ __attribute__((aligned(16))) unsigned char smem_tn[];
// `wave` = this wave's index among the n_waves that share the set's rows (k_matvec_tn: all waves of the launch; k_matvec_tn_mix: the waves of one of its two sets)
template <int T, int NU, int TN, int PRO>
__device__ __forceinline__ void matvec_tn_run(const MatSet &ms, const ActQ &A, const int N, const int ldy, const int n_groups, const int n_waves, const int wave, const ProArgs &pa,
                                              const int ldx, const int image_bytes) {
    static_assert(PRO == 0 || NU <= 3, "the prologue variant: 512-thread workgroups, K <= 3 x 64 units");
    using X = Tr<T>;
    const int lane = threadIdx.x & 63;
    const int K = ms.w0.cols, U = K / X::EPU, rows_each = ms.rows_each, total_rows = ms.n * rows_each;
    int uc[NU]; bool ok[NU];
#pragma unroll
    for (int i = 0; i < NU; i++) { const int u = lane + 64 * i; ok[i] = u < U; uc[i] = ok[i] ? u : 0; }
    struct Grp { typename X::WU w[NU]; float res[TN]; };
    const bool has_res = ms.res0 != nullptr;
    const float *res_base = has_res ? ms.res0 : ms.y0;
    const long long res_stride = has_res ? ms.dres : ms.dy;
    auto fetch = [&](int g, Grp &G) {           // every load unconditional (clamped indices): see matvec_run
        const int row = min(g, total_rows - 1);
        MG4_MATSET_ROW(X, ms, row, rows_each, U, B);
#pragma unroll
        for (int i = 0; i < NU; i++) X::loadb(B, uc[i], G.w[i]);
        const float *rb = MG4_MATSET_RES(res_base, res_stride);
#pragma unroll
        for (int t = 0; t < TN; t++) G.res[t] = load_res(rb + (size_t)min(t, N - 1) * ldy);
    };
    Grp cur, nxt;
    MG4_TL(0); MG4_TL_ALL(7);
    constexpr int PRND = PRO ? NU : 1;                                   // 512 threads x 4 elements per round: K <= NU * 2048
    float4 pxv[PRO ? TN : 1][PRND], pyv[PRND];
    bool pin[PRND];
    if (PRO) {   // the rows are requested before the first weight tiles (vector-memory results return in issue order)
#pragma unroll
        for (int r = 0; r < PRND; r++) {
            const int i = (r * 512 + (int)threadIdx.x) * 4;
            pin[r] = i < K;
            const int ic = pin[r] ? i : 0;
            pyv[r] = PRO == 1 ? *reinterpret_cast<const float4 *>(pa.w + ic) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
#pragma unroll
            for (int t = 0; t < (PRO ? TN : 1); t++) pxv[t][r] = *reinterpret_cast<const float4 *>(pa.x + (size_t)min(t, N - 1) * ldx + ic);
        }
    }
    fetch(wave, cur);
    MG4_TL(1);
    // K <= 3 x 64 units: every lane works on the SAME units of every weight row, so the TN activation fragments live in registers for the whole launch (no LDS
    // image, no barrier, no LDS re-read per weight row -- the LDS variant below re-reads TN x 5 KB per 3.5 KB weight row and is LDS-bandwidth bound).
    constexpr bool REG = mv_tn_reg<NU, TN>();
    typename X::AU ar[REG ? TN : 1][REG ? NU : 1];
    if (REG && PRO) {
        constexpr int mask = (T == GT_Q4_K || T == GT_Q5_K || T == GT_Q6_K) ? ACT_Q8K : ACT_Q80;
        double *red = reinterpret_cast<double *>(smem_tn);               // [TN][8 waves]
        if (PRO == 1) {
#pragma unroll
            for (int t = 0; t < (PRO ? TN : 1); t++) {
                double sum = 0.0;
#pragma unroll
                for (int r = 0; r < PRND; r++) {
                    const float4 v = pxv[t][r];
                    double q = 0.0;
                    MG4_ROW_SUMSQ4(q, v);
                    sum += pin[r] ? q : 0.0;
                }
                sum = wave_sum_d(sum);
                if (lane == 0) red[t * 8 + (threadIdx.x >> 6)] = sum;   // row_partial as text: called as a function, these kernels (and only these) compile differently
            }
            __syncthreads();
        }
        ActQ Li[PRO ? TN : 1];
#pragma unroll
        for (int t = 0; t < (PRO ? TN : 1); t++) {
            float scale = 1.0f;
            if (PRO == PRO_RMS) scale = row_scale(row_mean(row_total(red + t * 8, 8), K));
            ActQ L{};
            row_image(L, smem_tn + 512 + (size_t)t * image_bytes, K);
            L.bsq = nullptr; L.xh = nullptr; L.xf = nullptr;
#pragma unroll
            for (int r = 0; r < PRND; r++) {
                const int i = (r * 512 + (int)threadIdx.x) * 4;
                float v[4];
                row_value4<PRO == PRO_RMS ? PRO_RMS : PRO_PLAIN>(v, pxv[t][r], pyv[r], scale);   // PRO_PLAIN: the rows as they are (attention output -> wo)
                row_zero_unless(v, pin[r]);
                quant_emit4(v, pin[r], i, 0, K, L, mask);
            }
            Li[t] = L;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < (PRO ? TN : 1); t++)
#pragma unroll
            for (int i = 0; i < NU; i++) X::loada(Li[t], 0, K, uc[i], ar[REG ? t : 0][REG ? i : 0]);
    } else if (REG) {
#pragma unroll
        for (int t = 0; t < TN; t++)
#pragma unroll
            for (int i = 0; i < NU; i++) X::loada(A, min(t, N - 1), K, uc[i], ar[REG ? t : 0][REG ? i : 0]);
    }
    // otherwise: LDS image of the N activation rows, laid out like the global ActQ planes (so Tr<T>::loada indexes it unchanged)
    ActQ L;
    if (!REG) {
        unsigned char *p = smem_tn;
        const int nthr = (int)blockDim.x, tid = (int)threadIdx.x;
        // LDS-DMA copy (global_load_lds, 16 bytes per lane, destination lane-linear = a plain contiguous copy): all pieces of all planes are in flight together; the
        // round-1 form (a load -> ds_write loop, one dependent round trip per 4-8 KB) cost 14 serial round trips for a K = 13824 image -- most of the kernel's time.
        const int nwv = nthr >> 6, wv = tid >> 6;
        auto copy16 = [&](void *dst, const void *src, size_t bytes) {      // bytes is a multiple of 16 for every plane x row count used here, except the tails handled below
            const size_t n1k = (bytes + 1023) / 1024;
            for (size_t c = (size_t)wv; c < n1k; c += (size_t)nwv) {
                const size_t off = c * 1024 + (size_t)lane * 16;
                if (off + 16 <= bytes)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(reinterpret_cast<const unsigned char *>(src) + off),
                                                     (__attribute__((address_space(3))) void *)(reinterpret_cast<unsigned char *>(dst) + c * 1024), 16, 0, 0);
            }
            const size_t n16 = bytes / 16;
            for (size_t i = n16 * 16 + (size_t)tid; i < bytes; i += (size_t)nthr) reinterpret_cast<unsigned char *>(dst)[i] = reinterpret_cast<const unsigned char *>(src)[i];
        };
        if (tr_is_kquant<T>()) {
            L.q8k = reinterpret_cast<int8_t *>(p); p += (size_t)TN * K;
            L.dk = reinterpret_cast<float *>(p); p += (size_t)TN * (K / 256) * 4;
            L.bsk = reinterpret_cast<int16_t *>(p);
            copy16(L.q8k, A.q8k, (size_t)N * K); copy16(L.dk, A.dk, (size_t)N * (K / 256) * 4); copy16(L.bsk, A.bsk, (size_t)N * (K / 16) * 2);
        } else {
            L.q80 = reinterpret_cast<int8_t *>(p); p += (size_t)TN * K;
            L.d0 = reinterpret_cast<float *>(p); p += (size_t)TN * (K / 32) * 4;
            L.d1 = reinterpret_cast<float *>(p); p += (size_t)TN * (K / 32) * 4;
            L.s1 = reinterpret_cast<float *>(p); p += (size_t)TN * (K / 32) * 4;
            L.sum0 = reinterpret_cast<int *>(p);
            copy16(L.q80, A.q80, (size_t)N * K); copy16(L.d0, A.d0, (size_t)N * (K / 32) * 4); copy16(L.d1, A.d1, (size_t)N * (K / 32) * 4);
            copy16(L.s1, A.s1, (size_t)N * (K / 32) * 4); copy16(L.sum0, A.sum0, (size_t)N * (K / 32) * 4);
        }
    }
    if (!REG) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); }
    MG4_TL(2);
    auto consume = [&](int g, const Grp &G) {
        float out[TN];
#pragma unroll
        for (int t = 0; t < TN; t++) out[t] = 0.0f;
        // unit-major: the decoded weight unit (nibble / high-bit unpacking, scale extraction) is shared by the TN rows; per row the units are still
        // accumulated in index order, like the single-row kernel
#pragma unroll
        for (int i = 0; i < NU; i++) {
#pragma unroll
            for (int t = 0; t < TN; t++) {
                float c = out[t];
                if (REG) X::dot(G.w[i], ar[REG ? t : 0][REG ? i : 0], c);
                else { typename X::AU a; X::loada(L, min(t, N - 1), K, uc[i], a); X::dot(G.w[i], a, c); }
                out[t] = ok[i] ? c : out[t];
            }
        }
#pragma unroll
        for (int t = 0; t < TN; t++) out[t] = wave_sum(out[t]);
        if (lane == 0 && g < total_rows) {
            MG4_MATSET_M_LR(g, rows_each);
            float *yo = ms.y0 + (long long)m * ms.dy + lr;
#pragma unroll
            for (int t = 0; t < TN; t++) if (t < N) yo[(size_t)t * ldy] = has_res ? out[t] + G.res[t] : out[t];
        }
    };
    for (int g = wave; g < n_groups;) {
        fetch(g + n_waves, nxt);
        __builtin_amdgcn_sched_barrier(0);
        consume(g, cur);
        __builtin_amdgcn_sched_barrier(0);
#ifdef MG4_TIMELINE
        if (g == wave) MG4_TL(3);
#endif
        g += n_waves;
        if (g >= n_groups) break;
        fetch(g + n_waves, cur);
        __builtin_amdgcn_sched_barrier(0);
        consume(g, nxt);
        __builtin_amdgcn_sched_barrier(0);
        g += n_waves;
    }
    MG4_TL(4);
#ifdef MG4_TIMELINE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    MG4_TL(5); MG4_TL_ALL(6);
#endif
}
template <int T, int NU, int TN, int PRO = 0>
__global__ __launch_bounds__(mv_tn_threads<NU>()) void k_matvec_tn(const MatSet ms, const ActQ A, const int N, const int ldy, const int n_groups, const int n_waves, const ProArgs pa,
                                                                   const int ldx, const int image_bytes) {
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    matvec_tn_run<T, NU, TN, PRO>(ms, A, N, ldy, n_groups, n_waves, wave, pa, ldx, image_bytes);
}
// Two sets of different k-quant types with the same K (wq|wk + wv of a "more bits" layer) against the same TN rows in ONE launch: the workgroups are split between
// the sets by bytes, like k_matvec_mix does for the single-row step.  Both types quantise their rows to Q8_K, so the in-launch preparation (PRO = 1) is the same code
// with the same barriers on both sides of the split (a workgroup is never divided: the split is at workgroup granularity).
template <int T1, int T2, int NU, int TN, int PRO>
__global__ __launch_bounds__(mv_tn_threads<NU>()) void k_matvec_tn_mix(const MatSet ms1, const MatSet ms2, const ActQ A, const int N, const int ldy, const int n_groups1, const int n_waves1,
                                                                       const int n_groups2, const int n_waves2, const ProArgs pa, const int ldx, const int image_bytes) {
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (wave < n_waves1) matvec_tn_run<T1, NU, TN, PRO>(ms1, A, N, ldy, n_groups1, n_waves1, wave, pa, ldx, image_bytes);
    else matvec_tn_run<T2, NU, TN, PRO>(ms2, A, N, ldy, n_groups2, n_waves2, wave - n_waves1, pa, ldx, image_bytes);
}
template <int T, int NU, int TN>
static void launch_tn_n(const MatSet &ms, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s, const float *px, const float *pw, int ldx) {
    const int n_groups = ms.n * ms.rows_each;
    constexpr int WPB = mv_tn_threads<NU>() / 64;
    const int n_blocks = std::min((n_groups + WPB - 1) / WPB, tune.cus), n_waves = n_blocks * WPB;
    ProArgs pa{}; pa.x = px; pa.w = pw;
    constexpr bool PRO_OK = units_have(mv_tn_pro_units<T>(), NU);
    if constexpr (PRO_OK) {
        if (px) {
            const int img = (int)mv_tn_image_bytes(ms.w0.cols);
            static bool attr1 = false;
            if (!attr1) { HIP_IGNORE(lds_optin_max(&k_matvec_tn<T, NU, TN, 1>));
                          HIP_IGNORE(lds_optin_max(&k_matvec_tn<T, NU, TN, 2>)); attr1 = true; }
            note_kernel("k_matvec_tn<%d, %d, %d, %d>", T, NU, TN, pw ? 1 : 2);
            if (pw) hipLaunchKernelGGL((k_matvec_tn<T, NU, TN, 1>), dim3((unsigned)n_blocks), dim3((unsigned)mv_tn_threads<NU>()), (size_t)512 + (size_t)TN * img, s, ms, A, N, ldy, n_groups, n_waves, pa, ldx, img);
            else hipLaunchKernelGGL((k_matvec_tn<T, NU, TN, 2>), dim3((unsigned)n_blocks), dim3((unsigned)mv_tn_threads<NU>()), (size_t)512 + (size_t)TN * img, s, ms, A, N, ldy, n_groups, n_waves, pa, ldx, img);
            return;
        }
    }
    note_kernel("k_matvec_tn<%d, %d, %d, 0>", T, NU, TN);
    const size_t lds = mv_tn_reg<NU, TN>() ? 0 : mv_tn_lds(T, ms.w0.cols, TN);
    static bool attr = false;
    if (!attr) { HIP_IGNORE(lds_optin_max(&k_matvec_tn<T, NU, TN, 0>)); attr = true; }
    hipLaunchKernelGGL((k_matvec_tn<T, NU, TN, 0>), dim3((unsigned)n_blocks), dim3((unsigned)mv_tn_threads<NU>()), lds, s, ms, A, N, ldy, n_groups, n_waves, pa, 0, 0);
}
template <int T>
static bool launch_tn_type(const MatSet &ms, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s, const float *px, const float *pw, int ldx) {
    return mv_for_units(mv_tn_units<T>(), (ms.w0.cols / Tr<T>::EPU + 63) / 64, [&](auto n) {
        mv_for_rows(N, [&](auto tn) { launch_tn_n<T, decltype(n)::value, decltype(tn)::value>(ms, A, N, ldy, tune, s, px, pw, ldx); }); });
}
// 2..4 activation rows against 1..3 same-type, same-shape, equally spaced matrices in ONE weight pass: y[m][t * ldy + r] = W_m[r] . act[t] (+ residual[m][t * ldy + r]).
// false -> shape / type outside the kernel's range (the caller falls back to launch_mul_mat per matrix).
bool launch_matvec_rows(const QWeight *const *W, float *const *y, const float *const *residual, int n, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s, const float *px, const float *pw, int ldx) {
    if (px && !matvec_rows_prologue_ok(W[0]->type, W[0]->cols)) return false;
    if (N < 1 || N > 4 || !matvec_prologue_supported(W[0]->type, W[0]->cols)) return false;
    if (mv_tn_lds(W[0]->type, W[0]->cols, 4) > 150 * 1024) return false;
    MatSet ms;
    if (!fill_matset(ms, W, y, residual, n)) return false;
    return for_weight_type(W[0]->type, [&](auto t) { return launch_tn_type<decltype(t)::value>(ms, A, N, ldy, tune, s, px, pw, ldx); });
}

template <int T1, int T2, int NU, int TN>
static void launch_tn_mix_n(const MatSet &m1, const MatSet &m2, double bytes1, double bytes2, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s, const float *px, const float *pw, int ldx) {
    static_assert(NU <= 3, "register-resident rows, the prologue's range");
    const int ng1 = m1.n * m1.rows_each, ng2 = m2.n * m2.rows_each;
    constexpr int WPB = mv_tn_threads<NU>() / 64;
    const int total = tune.cus;
    const int b1 = mv_split_blocks(ng1, bytes1, ng2, bytes2, total, WPB), nw1 = b1 * WPB, nw2 = (total - b1) * WPB;
    ProArgs pa{}; pa.x = px; pa.w = pw;
    const dim3 grid((unsigned)total), block((unsigned)mv_tn_threads<NU>());
    if (px) {
        const int img = (int)mv_tn_image_bytes(m1.w0.cols);
        static bool attr1 = false;
        if (!attr1) { HIP_IGNORE(lds_optin_max(&k_matvec_tn_mix<T1, T2, NU, TN, 1>)); attr1 = true; }
        note_kernel("k_matvec_tn_mix<%d, %d, %d, %d, 1>", T1, T2, NU, TN);
        hipLaunchKernelGGL((k_matvec_tn_mix<T1, T2, NU, TN, 1>), grid, block, (size_t)512 + (size_t)TN * img, s, m1, m2, A, N, ldy, ng1, nw1, ng2, nw2, pa, ldx, img);
        return;
    }
    note_kernel("k_matvec_tn_mix<%d, %d, %d, %d, 0>", T1, T2, NU, TN);
    hipLaunchKernelGGL((k_matvec_tn_mix<T1, T2, NU, TN, 0>), grid, block, 0, s, m1, m2, A, N, ldy, ng1, nw1, ng2, nw2, pa, 0, 0);
}
template <int T1, int T2>
static bool launch_tn_mix_type(const MatSet &m1, const MatSet &m2, double b1, double b2, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s, const float *px, const float *pw, int ldx) {
    return mv_for_units(TnMixUnits{}, (m1.w0.cols / 32 + 63) / 64, [&](auto n) {
        mv_for_rows(N, [&](auto tn) { launch_tn_mix_n<T1, T2, decltype(n)::value, decltype(tn)::value>(m1, m2, b1, b2, A, N, ldy, tune, s, px, pw, ldx); }); });
}
// Batched decode, N = 1..4 rows: two sets of different k-quant types with the same K (wq|wk + wv of a "more bits" layer) in ONE launch.  px != null: the rows are
// prepared inside the launch (rms_norm(px_t) * pw, quantised), as in launch_matvec_rows.  false: outside the kernel's range, nothing was launched.
bool launch_matvec_rows_mixed(const QWeight *const *W1, float *const *y1, int n1, const QWeight *const *W2, float *const *y2, int n2, const ActQ &A, int N, int ldy, const LaunchTuning &tune, hipStream_t s,
                              const float *px, const float *pw, int ldx) {
    if (N < 1 || N > 4 || W1[0]->cols != W2[0]->cols || W1[0]->cols % 256 || W1[0]->cols / 32 > 3 * 64) return false;
    if (px && (!pw || !matvec_rows_prologue_ok(W1[0]->type, W1[0]->cols) || !matvec_rows_prologue_ok(W2[0]->type, W2[0]->cols))) return false;
    MatSet m1, m2;
    if (!fill_matset(m1, W1, y1, nullptr, n1) || !fill_matset(m2, W2, y2, nullptr, n2)) return false;
    double b1 = 0, b2 = 0;
    for (int i = 0; i < n1; i++) b1 += (double)W1[i]->bytes;
    for (int i = 0; i < n2; i++) b2 += (double)W2[i]->bytes;
    return for_mixed_types(W1[0]->type, W2[0]->type, [&](auto t1, auto t2) {
        return launch_tn_mix_type<decltype(t1)::value, decltype(t2)::value>(m1, m2, b1, b2, A, N, ldy, tune, s, px, pw, ldx); });
}

// Unquantised (F16) weights, prefill: ggml converts the activation rows to fp16 and accumulates exact fp16 products in fp32 (ggml_vec_dot_f16) -- which is
// precisely the vision tower's MFMA GEMM (v_mfma_f32_32x32x16_f16, fp32 accumulators), so rows >= 16 go there: BASELINE.json configs[4]
// (13B f16, 512-token prefill) is MFMA-bound instead of re-streaming 25 GB of weights once per 4 tokens.
void launch_mul_mat(const QWeight &W, const ActQ &A, int N, float *y, int ldy, const float *residual, const LaunchTuning &tune, hipStream_t s) {
    if (tune.mmq >= 2 && N >= 5 && (A.bsq || W.type == GT_Q4_0) && mmq2_supported(W.type, W.rows, W.cols)) {
        const QWeight *Wp[1] = {&W}; float *Yp[1] = {y}; const float *Rp[1] = {residual};
        if (launch_mmq2_set(Wp, Yp, residual ? Rp : nullptr, 1, A, N, ldy, tune, s)) return;
    }
    if (W.type == GT_F16 && N >= 16 && W.cols % 8 == 0) { launch_gemm_f16(A.xh, W.cols, reinterpret_cast<const __half *>(W.qs), W.cols, N, W.rows, W.cols, nullptr, residual, false, Tables{}, y, nullptr, ldy, tune, s); return; }
    if (!for_weight_type(W.type, [&](auto t) { launch_mul_mat_t<decltype(t)::value>(W, A, N, y, ldy, residual, s); return true; }))
        throw HipError{hipErrorInvalidValue, "unsupported weight type", __FILE__, __LINE__};
}


constexpr int RQ_THREADS = 1024;
__global__ __launch_bounds__(RQ_THREADS) void k_rms_quant(const float *__restrict__ x, const float *__restrict__ w, const int K, const ActQ A, const int mask, const int seq) {
    const size_t row = blockIdx.x;
    const float *xr = x + row * K;
    __shared__ double red[RQ_THREADS / 64];
    float scale = 1.0f;
    if (w && seq) {   // MINIGPT4_PARITY: the oracle's mean.  Two arms on purpose: with one arm and the choice at the mean, the plain path compiles to different code
        double sum = 0.0;
        for (int i = threadIdx.x * 4; i < K; i += RQ_THREADS * 4) { const float4 v = *reinterpret_cast<const float4 *>(xr + i); MG4_ROW_SUMSQ4(sum, v); }
        row_partial(red, sum);
        __syncthreads();
        scale = row_scale(row_mean_oracle(row_total(red, RQ_THREADS / 64), K, xr, red));
    } else if (w) {
        double sum = 0.0;
        for (int i = threadIdx.x * 4; i < K; i += RQ_THREADS * 4) { const float4 v = *reinterpret_cast<const float4 *>(xr + i); MG4_ROW_SUMSQ4(sum, v); }
        row_partial(red, sum);
        __syncthreads();
        scale = row_scale(row_mean(row_total(red, RQ_THREADS / 64), K));
    }
    for (int i0 = 0; i0 < K; i0 += RQ_THREADS * 4) {
        const int i = i0 + threadIdx.x * 4;
        const bool in = i < K;
        float v[4] = {0, 0, 0, 0};
        if (in) { const float4 xv = *reinterpret_cast<const float4 *>(xr + i);
            if (w) row_value4<PRO_RMS>(v, xv, *reinterpret_cast<const float4 *>(w + i), scale);
            else row_value4<PRO_PLAIN>(v, xv, xv, scale); }
        quant_emit4(v, in, i, row, K, A, mask);
    }
}
// Consumers of a split-K mat-mul whose combine step was deferred (round 3; SlabSrc in kernels.hpp): the value of element i of matrix m is
//     (slab_0[i] + slab_1[i] + ... + slab_{ks-1}[i]) (+ residual[i])          -- exactly k_mmq2_reduce_set's additions, in its order --
// formed where it is consumed instead of by a launch of its own (a prompt pass had 3.5 such launches per layer: 0.73 of the 142-row pass's 11.3 ms).
__device__ __forceinline__ float4 slab_sum4(const float *__restrict__ base, int ks, long long stride, const float *__restrict__ res, size_t i) {
    float4 s = *reinterpret_cast<const float4 *>(base + i);
    for (int z = 1; z < ks; z++) { const float4 t = *reinterpret_cast<const float4 *>(base + (size_t)z * stride + i); s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
    if (res) { const float4 t = *reinterpret_cast<const float4 *>(res + i); s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
    return s;
}
// x_out = residual + sum of slabs (the residual stream, materialised here), then k_rms_quant's norm + quantisation of the row
__global__ __launch_bounds__(RQ_THREADS) void k_rms_quant_slabs(const float *__restrict__ slabs, const int ks, const long long stride, const float *res, float *x_out,
                                                                const float *__restrict__ w, const int K, const ActQ A, const int mask) {
    const size_t row = blockIdx.x;
    float *xr = x_out + row * K;
    __shared__ double red[RQ_THREADS / 64];
    double sum = 0.0;
    for (int i = threadIdx.x * 4; i < K; i += RQ_THREADS * 4) {
        const float4 v = slab_sum4(slabs, ks, stride, res, row * K + i);
        *reinterpret_cast<float4 *>(xr + i) = v;                   // re-read below by the same thread
        MG4_ROW_SUMSQ4(sum, v);
    }
    row_partial(red, sum);
    __syncthreads();
    const float scale = row_scale(row_mean(row_total(red, RQ_THREADS / 64), K));
    for (int i0 = 0; i0 < K; i0 += RQ_THREADS * 4) {
        const int i = i0 + threadIdx.x * 4;
        const bool in = i < K;
        float v[4] = {0, 0, 0, 0};
        if (in) row_value4<PRO_RMS>(v, *reinterpret_cast<const float4 *>(xr + i), *reinterpret_cast<const float4 *>(w + i), scale);
        quant_emit4(v, in, i, row, K, A, mask);
    }
}
void launch_rms_quant_slabs(const SlabSrc &src, const float *w, int N, int K, const ActQ &A, int mask, hipStream_t s) {
    note_kernel("k_rms_quant_slabs");
    hipLaunchKernelGGL(k_rms_quant_slabs, dim3((unsigned)N), dim3(RQ_THREADS), 0, s, src.ws, src.ks, src.stride, src.res[0], src.y[0], w, K, A, mask);
}
void launch_rms_quant(const float *x, const float *w, int N, int K, const ActQ &A, int mask, hipStream_t s, bool sequential_sum) {
    note_kernel("k_rms_quant");
    hipLaunchKernelGGL(k_rms_quant, dim3((unsigned)N), dim3(RQ_THREADS), 0, s, x, w, K, A, mask, sequential_sum ? 1 : 0);
}

__global__ __launch_bounds__(256) void k_silu_mul_quant(const float *__restrict__ a, const float *__restrict__ b, const int K, const ActQ A, const int mask, const Tables tb) {
    // (a, b, K) is the preloaded head: the two row loads wait for nothing.  Without preload every argument is requested in one batch at entry ("Kernel arguments", above matvec_run)
    if (MV_PIN_AT_ENTRY) asm volatile("" ::"s"(a), "s"(b), "s"(K), "s"(mask), "s"(tb.silu), "s"(A.q8k), "s"(A.dk), "s"(A.bsk), "s"(A.bsq), "s"(A.q80), "s"(A.d0), "s"(A.d1), "s"(A.s1), "s"(A.sum0));
    const size_t row = blockIdx.y;
    const int i = blockIdx.x * 1024 + threadIdx.x * 4;
    const bool in = i < K;
    float v[4] = {0, 0, 0, 0};
    if (in) { const float4 av = *reinterpret_cast<const float4 *>(a + row * K + i);
        if (b) { const float4 bv = *reinterpret_cast<const float4 *>(b + row * K + i);
            v[0] = silu_h(tb.silu, av.x) * bv.x; v[1] = silu_h(tb.silu, av.y) * bv.y; v[2] = silu_h(tb.silu, av.z) * bv.z; v[3] = silu_h(tb.silu, av.w) * bv.w; }
        else { v[0] = av.x; v[1] = av.y; v[2] = av.z; v[3] = av.w; } }
    quant_emit4(v, in, i, row, K, A, mask);
}
// a = sum of matrix 0's slabs, b = sum of matrix 1's (w1 | w3 of a prompt pass): neither product is written out
__global__ __launch_bounds__(256) void k_silu_mul_quant_slabs(const float *__restrict__ slabs, const int ks, const long long stride, const int K, const ActQ A, const int mask, const Tables tb) {
    const size_t row = blockIdx.y;
    const int i = blockIdx.x * 1024 + threadIdx.x * 4;
    const bool in = i < K;
    float v[4] = {0, 0, 0, 0};
    if (in) {
        const float4 av = slab_sum4(slabs, ks, stride, nullptr, row * K + i), bv = slab_sum4(slabs + (size_t)ks * stride, ks, stride, nullptr, row * K + i);
        v[0] = tab(tb.silu, av.x) * bv.x; v[1] = tab(tb.silu, av.y) * bv.y; v[2] = tab(tb.silu, av.z) * bv.z; v[3] = tab(tb.silu, av.w) * bv.w;
    }
    quant_emit4(v, in, i, row, K, A, mask);
}
void launch_silu_mul_quant_slabs(const SlabSrc &src, int N, int K, const ActQ &A, int mask, const Tables &tb, hipStream_t s) {
    note_kernel("k_silu_mul_quant_slabs");
    hipLaunchKernelGGL(k_silu_mul_quant_slabs, dim3((unsigned)((K + 1023) / 1024), (unsigned)N), dim3(256), 0, s, src.ws, src.ks, src.stride, K, A, mask, tb);
}
void launch_silu_mul_quant(const float *a, const float *b, int N, int K, const ActQ &A, int mask, const Tables &tb, hipStream_t s) {
    note_kernel("k_silu_mul_quant");
    hipLaunchKernelGGL(k_silu_mul_quant, dim3((unsigned)((K + 1023) / 1024), (unsigned)N), dim3(256), 0, s, a, b, K, A, mask, tb);
}

// =====================================================================================================================
// embedding gather: dequantise rows of the raw (un-repacked) ggml table
// =====================================================================================================================
__device__ __forceinline__ void sm_k4(int j, const uint8_t *q, int &d, int &m) {
    if (j < 4) { d = q[j] & 63; m = q[j + 4] & 63; } else { d = (q[j + 4] & 0xF) | ((q[j - 4] >> 6) << 4); m = (q[j + 4] >> 4) | ((q[j] >> 6) << 4); }
}
__device__ float dequant_elem(int type, const uint8_t *row, int e) {
    switch (type) {
    case GT_F32: return reinterpret_cast<const float *>(row)[e];
    case GT_F16: return h2f_bits(reinterpret_cast<const unsigned short *>(row)[e]);
    case GT_Q4_0: { const uint8_t *b = row + (e >> 5) * 18; const int j = e & 31; const float d = h2f_bits(b[0] | (b[1] << 8)); const int q = j < 16 ? (b[2 + j] & 15) : (b[2 + j - 16] >> 4); return (float)(q - 8) * d; }
    case GT_Q4_1: { const uint8_t *b = row + (e >> 5) * 20; const int j = e & 31; const float d = h2f_bits(b[0] | (b[1] << 8)), m = h2f_bits(b[2] | (b[3] << 8)); const int q = j < 16 ? (b[4 + j] & 15) : (b[4 + j - 16] >> 4); return (float)q * d + m; }
    case GT_Q5_0: { const uint8_t *b = row + (e >> 5) * 22; const int j = e & 31; const float d = h2f_bits(b[0] | (b[1] << 8)); const unsigned qh = b[2] | (b[3] << 8) | (b[4] << 16) | ((unsigned)b[5] << 24);
        const int q = (j < 16 ? (b[6 + j] & 15) : (b[6 + j - 16] >> 4)) | (((qh >> j) & 1) << 4); return (float)(q - 16) * d; }
    case GT_Q5_1: { const uint8_t *b = row + (e >> 5) * 24; const int j = e & 31; const float d = h2f_bits(b[0] | (b[1] << 8)), m = h2f_bits(b[2] | (b[3] << 8)); const unsigned qh = b[4] | (b[5] << 8) | (b[6] << 16) | ((unsigned)b[7] << 24);
        const int q = (j < 16 ? (b[8 + j] & 15) : (b[8 + j - 16] >> 4)) | (((qh >> j) & 1) << 4); return (float)q * d + m; }
    case GT_Q8_0: { const uint8_t *b = row + (e >> 5) * 34; const float d = h2f_bits(b[0] | (b[1] << 8)); return (float)(signed char)b[2 + (e & 31)] * d; }
    case GT_Q2_K: { const uint8_t *b = row + (e >> 8) * 84; const int i = e & 255, n = i >> 7, j = (i >> 5) & 3, l = i & 31; const uint8_t sc = b[i >> 4];
        const float d = h2f_bits(b[80] | (b[81] << 8)), dm = h2f_bits(b[82] | (b[83] << 8)); const float dl = d * (float)(sc & 0xF), ml = dm * (float)(sc >> 4);
        return dl * (float)((b[16 + 32 * n + l] >> (2 * j)) & 3) - ml; }
    case GT_Q4_K: { const uint8_t *b = row + (e >> 8) * 144; const int i = e & 255, s = i >> 5, l = i & 31; const float d = h2f_bits(b[0] | (b[1] << 8)), dm = h2f_bits(b[2] | (b[3] << 8)); int sc, m; sm_k4(s, b + 4, sc, m);
        const uint8_t qb = b[16 + (s >> 1) * 32 + l]; const int q = (s & 1) ? (qb >> 4) : (qb & 15); return (d * sc) * (float)q - dm * m; }
    case GT_Q5_K: { const uint8_t *b = row + (e >> 8) * 176; const int i = e & 255, s = i >> 5, l = i & 31; const float d = h2f_bits(b[0] | (b[1] << 8)), dm = h2f_bits(b[2] | (b[3] << 8)); int sc, m; sm_k4(s, b + 4, sc, m);
        const uint8_t qb = b[48 + (s >> 1) * 32 + l]; const int q = ((s & 1) ? (qb >> 4) : (qb & 15)) + (((b[16 + l] >> s) & 1) ? 16 : 0); return (d * sc) * (float)q - dm * m; }
    case GT_Q6_K: { const uint8_t *b = row + (e >> 8) * 210; const int i = e & 255, n = i >> 7, a = (i >> 5) & 3, l = i & 31; const float d = h2f_bits(b[208] | (b[209] << 8));
        const uint8_t qlb = b[64 * n + 32 * (a & 1) + l]; const int lo = (a & 2) ? (qlb >> 4) : (qlb & 15); const int hi = (b[128 + 32 * n + l] >> (2 * a)) & 3;
        const int q = (lo | (hi << 4)) - 32; const int sc = (signed char)b[192 + 8 * n + 2 * a + (l >> 4)]; return d * (float)sc * (float)q; }
    default: return 0.0f;
    }
}
constexpr int GR_THREADS = 256;
__global__ __launch_bounds__(GR_THREADS) void k_get_rows(int type, const uint8_t *__restrict__ table, int K, size_t row_bytes, const int *__restrict__ tokens, float *__restrict__ out) {
    if (MV_PIN_AT_ENTRY) asm volatile("" ::"s"(type), "s"(table), "s"(K), "s"(row_bytes), "s"(tokens), "s"(out));   // one batch; the token id itself lives in device memory
    const int t = blockIdx.x;
    if (tokens[t] < 0) return;                     // embedding row: already written by the host copy
    const uint8_t *row = table + (size_t)tokens[t] * row_bytes;
    const int e = blockIdx.y * GR_THREADS + threadIdx.x;   // the workgroup size as a constant: blockDim.x is a hidden kernel argument, a scalar load of its own
    if (e < K) out[(size_t)t * K + e] = dequant_elem(type, row, e);
}
void launch_get_rows(int type, const uint8_t *raw_table, int K, const int *tokens, int N, float *out, hipStream_t s) {
    note_kernel("k_get_rows");
    hipLaunchKernelGGL(k_get_rows, dim3((unsigned)N, (unsigned)((K + GR_THREADS - 1) / GR_THREADS)), dim3(GR_THREADS), 0, s, type, raw_table, K, gt_nbytes(type, (size_t)K), tokens, out);
}

// =====================================================================================================================
// RoPE (ggml mode 0: interleaved pairs; cos/sin table built on the host with ggml's iterative fp32 theta) + KV append
// =====================================================================================================================
__global__ void k_rope_kv(float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, int E, int hd, const int *__restrict__ n_past,
                          const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, __half *__restrict__ kc, __half *__restrict__ vc) {
    const int t = blockIdx.x, h = blockIdx.y, i = threadIdx.x;   // i < hd/2
    const int pos = *n_past + t;
    const float c = cos_tab[(size_t)pos * (hd / 2) + i], s = sin_tab[(size_t)pos * (hd / 2) + i];
    const size_t o = (size_t)t * E + (size_t)h * hd + 2 * i;
    const float q0 = q[o], q1 = q[o + 1];
    q[o] = q0 * c - q1 * s; q[o + 1] = q0 * s + q1 * c;
    const float k0 = k[o], k1 = k[o + 1];
    const size_t co = (size_t)pos * E + (size_t)h * hd + 2 * i;
    *reinterpret_cast<__half2 *>(kc + co) = __floats2half2_rn(k0 * c - k1 * s, k0 * s + k1 * c);
    *reinterpret_cast<__half2 *>(vc + co) = __floats2half2_rn(v[o], v[o + 1]);
}
// q | k | v = the sums of the three matrices' slabs (wq | wk | wv of a prompt pass); the rotated q is written to `q` as before, k and v only to the caches
struct RopeSlabs { const float *base[3]; int ks[3]; };
__global__ void k_rope_kv_slabs(const RopeSlabs rs, const long long stride, float *__restrict__ q, int E, int hd, const int *__restrict__ n_past,
                                const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, __half *__restrict__ kc, __half *__restrict__ vc) {
    const int t = blockIdx.x, h = blockIdx.y, i = threadIdx.x;   // i < hd/2
    const int pos = *n_past + t;
    const float c = cos_tab[(size_t)pos * (hd / 2) + i], s = sin_tab[(size_t)pos * (hd / 2) + i];
    const size_t o = (size_t)t * E + (size_t)h * hd + 2 * i;
    float2 m[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float *b = rs.base[a] + o;
        float2 acc = *reinterpret_cast<const float2 *>(b);
        for (int z = 1; z < rs.ks[a]; z++) { const float2 u = *reinterpret_cast<const float2 *>(b + (size_t)z * stride); acc.x += u.x; acc.y += u.y; }
        m[a] = acc;
    }
    q[o] = m[0].x * c - m[0].y * s; q[o + 1] = m[0].x * s + m[0].y * c;
    const size_t co = (size_t)pos * E + (size_t)h * hd + 2 * i;
    *reinterpret_cast<__half2 *>(kc + co) = __floats2half2_rn(m[1].x * c - m[1].y * s, m[1].x * s + m[1].y * c);
    *reinterpret_cast<__half2 *>(vc + co) = __floats2half2_rn(m[2].x, m[2].y);
}
// Packed prompt rows of several conversations (Engine::prefill_batch): row t belongs to conversation rows[2 t] at position rows[2 t + 1]; its cache row is
// that position in the conversation's region, kc / vc + slot * seq_stride.  Otherwise the arithmetic of k_rope_kv / k_rope_kv_slabs, statement for statement.
__global__ void k_rope_kv_seg(float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, int E, int hd, const int *__restrict__ rows, long long seq_stride,
                              const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, __half *__restrict__ kc, __half *__restrict__ vc) {
    const int t = blockIdx.x, h = blockIdx.y, i = threadIdx.x;   // i < hd/2
    const int pos = rows[2 * t + 1];
    const float c = cos_tab[(size_t)pos * (hd / 2) + i], s = sin_tab[(size_t)pos * (hd / 2) + i];
    const size_t o = (size_t)t * E + (size_t)h * hd + 2 * i;
    const float q0 = q[o], q1 = q[o + 1];
    q[o] = q0 * c - q1 * s; q[o + 1] = q0 * s + q1 * c;
    const float k0 = k[o], k1 = k[o + 1];
    const size_t co = (size_t)rows[2 * t] * seq_stride + (size_t)pos * E + (size_t)h * hd + 2 * i;
    *reinterpret_cast<__half2 *>(kc + co) = __floats2half2_rn(k0 * c - k1 * s, k0 * s + k1 * c);
    *reinterpret_cast<__half2 *>(vc + co) = __floats2half2_rn(v[o], v[o + 1]);
}
__global__ void k_rope_kv_seg_slabs(const RopeSlabs rs, const long long stride, float *__restrict__ q, int E, int hd, const int *__restrict__ rows, long long seq_stride,
                                    const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, __half *__restrict__ kc, __half *__restrict__ vc) {
    const int t = blockIdx.x, h = blockIdx.y, i = threadIdx.x;   // i < hd/2
    const int pos = rows[2 * t + 1];
    const float c = cos_tab[(size_t)pos * (hd / 2) + i], s = sin_tab[(size_t)pos * (hd / 2) + i];
    const size_t o = (size_t)t * E + (size_t)h * hd + 2 * i;
    float2 m[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float *b = rs.base[a] + o;
        float2 acc = *reinterpret_cast<const float2 *>(b);
        for (int z = 1; z < rs.ks[a]; z++) { const float2 u = *reinterpret_cast<const float2 *>(b + (size_t)z * stride); acc.x += u.x; acc.y += u.y; }
        m[a] = acc;
    }
    q[o] = m[0].x * c - m[0].y * s; q[o + 1] = m[0].x * s + m[0].y * c;
    const size_t co = (size_t)rows[2 * t] * seq_stride + (size_t)pos * E + (size_t)h * hd + 2 * i;
    *reinterpret_cast<__half2 *>(kc + co) = __floats2half2_rn(m[1].x * c - m[1].y * s, m[1].x * s + m[1].y * c);
    *reinterpret_cast<__half2 *>(vc + co) = __floats2half2_rn(m[2].x, m[2].y);
}
void launch_rope_kv_slabs(const SlabSrc &src, int N, int n_head, int hd, const int *n_past, const float *cos_tab, const float *sin_tab, __half *kcache, __half *vcache, hipStream_t s) {
    RopeSlabs rs;
    for (int a = 0; a < 3; a++) { rs.base[a] = src.mbase[a]; rs.ks[a] = src.mks[a]; }
    hipLaunchKernelGGL(k_rope_kv_slabs, dim3((unsigned)N, (unsigned)n_head), dim3((unsigned)(hd / 2)), 0, s, rs, src.stride, src.y[0], n_head * hd, hd, n_past, cos_tab, sin_tab, kcache, vcache);
}
void launch_rope_kv(float *q, const float *k, const float *v, int N, int n_head, int hd, const int *n_past, const float *cos_tab, const float *sin_tab,
                    __half *kcache, __half *vcache, hipStream_t s) {
    hipLaunchKernelGGL(k_rope_kv, dim3((unsigned)N, (unsigned)n_head), dim3((unsigned)(hd / 2)), 0, s, q, k, v, n_head * hd, hd, n_past, cos_tab, sin_tab, kcache, vcache);
}
void launch_rope_kv_seg(float *q, const float *k, const float *v, int N, int n_head, int hd, const int *rows, size_t seq_stride, const float *cos_tab, const float *sin_tab,
                        __half *kcache, __half *vcache, hipStream_t s) {
    note_kernel("k_rope_kv_seg");
    hipLaunchKernelGGL(k_rope_kv_seg, dim3((unsigned)N, (unsigned)n_head), dim3((unsigned)(hd / 2)), 0, s, q, k, v, n_head * hd, hd, rows, (long long)seq_stride, cos_tab, sin_tab, kcache, vcache);
}
void launch_rope_kv_seg_slabs(const SlabSrc &src, int N, int n_head, int hd, const int *rows, size_t seq_stride, const float *cos_tab, const float *sin_tab, __half *kcache, __half *vcache,
                              hipStream_t s) {
    RopeSlabs rs;
    for (int a = 0; a < 3; a++) { rs.base[a] = src.mbase[a]; rs.ks[a] = src.mks[a]; }
    note_kernel("k_rope_kv_seg_slabs");
    hipLaunchKernelGGL(k_rope_kv_seg_slabs, dim3((unsigned)N, (unsigned)n_head), dim3((unsigned)(hd / 2)), 0, s, rs, src.stride, src.y[0], n_head * hd, hd, rows, (long long)seq_stride, cos_tab,
                       sin_tab, kcache, vcache);
}
// The table k_rope_kv reads, exactly ggml's iteration: theta = pos; theta *= theta_scale per pair (fp32), cosf/sinf.  [n_ctx][hd / 2] each
void rope_tables(int n_ctx, int hd, std::vector<float> &c, std::vector<float> &s) {
    const size_t C = (size_t)n_ctx, P = (size_t)hd / 2;
    c.assign(C * P, 0.0f); s.assign(C * P, 0.0f);
    const float theta_scale = powf(10000.0f, -2.0f / (float)hd);
    for (size_t p = 0; p < C; p++) { float theta = (float)p; for (size_t i = 0; i < P; i++) { c[p * P + i] = cosf(theta); s[p * P + i] = sinf(theta); theta *= theta_scale; } }
}

// =====================================================================================================================
// Context shift: rows [n_keep + n_discard, n_rows) of one conversation's caches move down by n_discard, in place; the moved keys are rotated by
// -n_discard positions (RoPE is relative: a key rotated to position p, then by -d, is the key at p - d up to the fp16 rounding of both steps).
// Lane = (K or V, layer, 16-byte column group): it owns that column of every row of its layer and walks the rows upwards in batches of
// b = min(n_discard, KV_SHIFT_ROWS).  All sources of a batch are loaded before any destination is stored; with b <= n_discard the destinations
// lie below the batch's sources, and later batches only read rows above every row written so far -- correct for every n_discard >= 1.  A
// wave's 64 lanes cover 1 KiB of one row (coalesced 16-byte accesses); the kernel is a pure HBM stream.
// =====================================================================================================================
constexpr int KV_SHIFT_ROWS = 8, KV_SHIFT_THREADS = 64;
__global__ __launch_bounds__(KV_SHIFT_THREADS) void k_kv_shift(__half *__restrict__ kc, __half *__restrict__ vc, int n_layer, int n_ctx, int E, int hd, int n_keep,
                                                             int n_discard, int n_rows, const float *__restrict__ cos_tab, const float *__restrict__ sin_tab) {
    const int G = E / 8;                                                   // 16-byte column groups per row
    const long long per = (long long)n_layer * G;
    const long long lane = (long long)blockIdx.x * KV_SHIFT_THREADS + threadIdx.x;
    if (lane >= 2 * per) return;
    const bool is_k = lane < per;
    const long long lg = is_k ? lane : lane - per;
    const int layer = (int)(lg / G), g = (int)(lg % G);
    __half *col = (is_k ? kc : vc) + (size_t)layer * n_ctx * E + (size_t)g * 8;
    float c[4] = {1.0f, 1.0f, 1.0f, 1.0f}, s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (is_k) {                                                            // a group's 4 pairs lie inside one head (hd % 8 == 0)
        const size_t t0 = (size_t)n_discard * (hd / 2) + (size_t)((g * 8) % hd) / 2;
#pragma unroll
        for (int j = 0; j < 4; j++) { c[j] = cos_tab[t0 + j]; s[j] = sin_tab[t0 + j]; }
    }
    const int b = min(n_discard, KV_SHIFT_ROWS);
    for (int r0 = n_keep + n_discard; r0 < n_rows; r0 += b) {
        const int nb = min(b, n_rows - r0);
        uint4 buf[KV_SHIFT_ROWS];
#pragma unroll
        for (int t = 0; t < KV_SHIFT_ROWS; t++) if (t < nb) buf[t] = *reinterpret_cast<const uint4 *>(col + (size_t)(r0 + t) * E);
#pragma unroll
        for (int t = 0; t < KV_SHIFT_ROWS; t++) {
            if (t >= nb) continue;
            uint4 u = buf[t];
            if (is_k) {
                unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    // fp16 x fp32 products are exact in double: the sum is rounded once (then to fp16, within one fp16 ulp of the exact rotation even where
                    // the two terms cancel -- fp32 products would not be)
                    const float2 kf = __half22float2(*reinterpret_cast<const __half2 *>(&w[j]));
                    const double k0 = kf.x, k1 = kf.y, cj = c[j], sj = s[j];
                    const __half2 r = __floats2half2_rn((float)(k0 * cj + k1 * sj), (float)(k1 * cj - k0 * sj));
                    w[j] = *reinterpret_cast<const unsigned *>(&r);
                }
                u = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4 *>(col + (size_t)(r0 + t - n_discard) * E) = u;
        }
    }
}
void launch_kv_shift(__half *kc_slot, __half *vc_slot, int n_layer, int n_ctx, int E, int hd, int n_keep, int n_discard, int n_rows, const float *cos_tab,
                     const float *sin_tab, hipStream_t s) {
    if (n_discard < 1 || n_keep < 0 || n_keep + n_discard >= n_rows) return;   // no row moves
    if (n_rows > n_ctx || n_discard > n_ctx - 1 || E % 8 || hd % 8 || E % hd) throw HipError{hipErrorInvalidValue, "launch_kv_shift: bad shape", __FILE__, __LINE__};
    note_kernel("k_kv_shift");
    const long long lanes = 2LL * n_layer * (E / 8);
    hipLaunchKernelGGL(k_kv_shift, dim3((unsigned)((lanes + KV_SHIFT_THREADS - 1) / KV_SHIFT_THREADS)), dim3(KV_SHIFT_THREADS), 0, s, kc_slot, vc_slot, n_layer, n_ctx, E, hd,
                       n_keep, n_discard, n_rows, cos_tab, sin_tab);
}

// =====================================================================================================================
// Prefix copy (Engine::fork, the prefix store): rows [0, n_rows) of every layer, keys and values, from ONE region with layer stride src_rows * E (a
// conversation's caches or the compact store) to n_dst regions with layer stride dst_rows * E.  Per layer and tensor the rows of a prefix are one
// contiguous run of n_rows * E halves, so the copy is 2 * n_layer runs cut into 16-byte pieces: lane t of workgroup b takes the pieces
// (b * KV_COPY_PIECES + j) * KV_COPY_THREADS + t, j < KV_COPY_PIECES -- every load of a wave is one coalesced KiB, all KV_COPY_PIECES loads are issued before
// the first store, and each piece is stored to every destination from the register it was loaded into (one-to-many: the source is read once).  The grid
// follows the byte count (45 rows of a 13B layer are 460 KB per tensor: a grid over layers alone would leave most of the device idle).  Plain stores: the
// written lines stay in the storing XCD's L2, and the next prompt pass reads exactly these rows.
// Destinations travel BY VALUE in the kernel arguments (KvCopyDst, 2 x 64 pointers = 1 KiB of the 4 KiB segment) rather than in a device table like
// d_seg_: a table would need a host-to-device copy and a wait for the previous use of its pinned staging before every launch, which costs more than the
// copy of a 45-row prefix itself; the argument segment is written by the launch.  The lanes index it uniformly (scalar loads from the constant segment).
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): 36 VGPRs, 30 SGPRs, no scratch, no LDS, occupancy 8 waves per SIMD.  The pieces are four named values,
// not an array: as an array the compiler kept them in LDS (16 KB per workgroup) and the loads were no longer in flight together.
// =====================================================================================================================
constexpr int KV_COPY_PIECES = 4, KV_COPY_THREADS = 256;
struct KvPiece { uint4 data; size_t off; int sel; };                       // off: destination offset in halves; sel: 0 = past the end (not stored), 1 = key, 2 = value
__device__ __forceinline__ KvPiece kv_piece_load(const __half *src_k, const __half *src_v, unsigned i0, unsigned total, unsigned per, unsigned n_layer, unsigned src_rows,
                                                 unsigned dst_rows, unsigned E) {
    const unsigned i = i0 < total ? i0 : 0u;                               // past the end: piece 0 is loaded (in bounds, total >= 1) and not stored
    const unsigned run = i / per, within = i - run * per;                  // run = tensor * n_layer + layer
    const bool is_v = run >= n_layer;
    const unsigned layer = is_v ? run - n_layer : run;
    KvPiece p;
    p.data = *reinterpret_cast<const uint4 *>((is_v ? src_v : src_k) + (size_t)layer * src_rows * E + (size_t)within * 8);
    p.off = (size_t)layer * dst_rows * E + (size_t)within * 8;
    p.sel = i0 < total ? (is_v ? 2 : 1) : 0;
    return p;
}
__device__ __forceinline__ void kv_piece_store(const KvPiece &p, __half *dk, __half *dv) {
    if (p.sel) *reinterpret_cast<uint4 *>((p.sel == 2 ? dv : dk) + p.off) = p.data;
}
// the source pointers are NOT __restrict__ on purpose: the loads then cannot be moved below (or repeated behind) the stores, so the four of a lane stay in flight together
__global__ __launch_bounds__(KV_COPY_THREADS) void k_kv_copy(const __half *src_k, const __half *src_v, unsigned src_rows, const KvCopyDst dst, int n_dst, unsigned dst_rows,
                                                           unsigned n_layer, unsigned E, unsigned n_rows) {
    static_assert(KV_COPY_PIECES == 4, "the four pieces are named");
    const unsigned per = n_rows * (E / 8);                                 // 16-byte pieces of one layer's run
    const unsigned total = 2u * n_layer * per;                             // < 2^31 (launch_kv_copy)
    const unsigned first = blockIdx.x * (KV_COPY_PIECES * KV_COPY_THREADS) + threadIdx.x;
    const KvPiece p0 = kv_piece_load(src_k, src_v, first, total, per, n_layer, src_rows, dst_rows, E);
    const KvPiece p1 = kv_piece_load(src_k, src_v, first + KV_COPY_THREADS, total, per, n_layer, src_rows, dst_rows, E);
    const KvPiece p2 = kv_piece_load(src_k, src_v, first + 2 * KV_COPY_THREADS, total, per, n_layer, src_rows, dst_rows, E);
    const KvPiece p3 = kv_piece_load(src_k, src_v, first + 3 * KV_COPY_THREADS, total, per, n_layer, src_rows, dst_rows, E);
    for (int d = 0; d < n_dst; d++) {
        __half *const dk = dst.k[d], *const dv = dst.v[d];
        kv_piece_store(p0, dk, dv); kv_piece_store(p1, dk, dv); kv_piece_store(p2, dk, dv); kv_piece_store(p3, dk, dv);
    }
}
void launch_kv_copy(const __half *src_k, const __half *src_v, int src_rows, const KvCopyDst &dst, int n_dst, int dst_rows, int n_layer, int E, int n_rows, hipStream_t s) {
    auto bad = [](const char *what) { throw HipError{hipErrorInvalidValue, what, __FILE__, __LINE__}; };
    if (!src_k || !src_v || n_dst < 1 || n_dst > KV_COPY_MAX_DST || n_layer < 1 || E < 8 || E % 8 || src_rows < 1 || dst_rows < 1 || n_rows < 0) bad("launch_kv_copy: bad shape");
    if (n_rows > src_rows || n_rows > dst_rows) bad("launch_kv_copy: n_rows exceeds a region's row count");
    auto aligned = [](const __half *p) { return (uintptr_t)p % 16 == 0; };   // the 16-byte accesses (with E % 8 every layer and row offset keeps the alignment)
    if (!aligned(src_k) || !aligned(src_v)) bad("launch_kv_copy: a region is not 16-byte aligned");
    const size_t src_n = (size_t)n_layer * src_rows * E, dst_n = (size_t)n_layer * dst_rows * E;
    auto overlap = [](const __half *a, size_t na, const __half *b, size_t nb) { const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b; return x < y + 2 * nb && y < x + 2 * na; };
    for (int d = 0; d < n_dst; d++) {
        if (!dst.k[d] || !dst.v[d]) bad("launch_kv_copy: bad shape");
        if (!aligned(dst.k[d]) || !aligned(dst.v[d])) bad("launch_kv_copy: a region is not 16-byte aligned");
        for (const __half *p : {dst.k[d], dst.v[d]}) if (overlap(p, dst_n, src_k, src_n) || overlap(p, dst_n, src_v, src_n)) bad("launch_kv_copy: a destination overlaps the source");
    }
    if (n_rows == 0) return;
    const unsigned long long total = 2ull * n_layer * n_rows * (E / 8);
    if (total >= (1ull << 31)) bad("launch_kv_copy: bad shape");
    note_kernel("k_kv_copy");
    const unsigned per_block = KV_COPY_PIECES * KV_COPY_THREADS;
    hipLaunchKernelGGL(k_kv_copy, dim3((unsigned)((total + per_block - 1) / per_block)), dim3(KV_COPY_THREADS), 0, s, src_k, src_v, (unsigned)src_rows, dst, n_dst, (unsigned)dst_rows,
                       (unsigned)n_layer, (unsigned)E, (unsigned)n_rows);
}

// =====================================================================================================================
// Snapshot pack / unpack (Engine::state_save / state_load): rows [r0, r0 + n) of ONE conversation's regions (kc / vc = [n_layer][n_ctx][E] fp16) <-> one contiguous
// block laid out [tensor K, V][layer][row][E], which k_kv_copy cannot express (it starts at row 0 and has no integrity check).  Per layer and tensor the rows are one
// contiguous run of n * E halves cut into 16-byte pieces, as in k_kv_copy; the block is the 2 * n_layer runs back to back, so piece i of the launch IS piece i of the block
// and only the cache side is strided (layer stride n_ctx * E).  Lane t of workgroup b takes the pieces (b * KV_COPY_PIECES + j) * KV_COPY_THREADS + t: every load and store
// of a wave is one coalesced KiB on both sides, the four loads of a lane are issued before its first store (pointers not __restrict__, as in k_kv_copy).
// The same sweep sums the block: the wrapping 64-bit sum of its 32-bit words (k_checksum's definition), taken from the registers the pieces were loaded into -- PACK sums
// what it stores into the block, UNPACK what it read from the block, so the two agree exactly when the block arrived unchanged.  Integer addition is order-free: the value
// does not depend on the grid.  Reduction: wave (shuffles), workgroup (one 8-byte LDS word per wave), then ONE 64-bit vector atomic add per workgroup into *sum, which the launcher
// zeroes in the stream before the launch (a 32 MiB block: 2048 adds).
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage), k_kv_pack | k_kv_unpack: 34 | 40 VGPRs, 28 | 28 SGPRs, no scratch, 32 bytes of LDS, occupancy 8 waves per SIMD.  The
// pieces are four named values, not an array: k_kv_copy's array ended up in LDS (16 KB per workgroup) and its loads were no longer in flight together.
// =====================================================================================================================
struct KvBlockPiece { uint4 data; size_t cache_off; unsigned idx; int sel; };   // cache_off: halves into the tensor's region; idx: piece of the block; sel as KvPiece
template <bool PACK>
__device__ __forceinline__ KvBlockPiece kv_block_load(const __half *kc, const __half *vc, const __half *blk, unsigned i0, unsigned total, unsigned per, unsigned n_layer,
                                                      unsigned n_ctx, unsigned E, unsigned r0) {
    const unsigned i = i0 < total ? i0 : 0u;                               // past the end: piece 0 is loaded (in bounds, total >= 1), neither stored nor summed
    const unsigned run = i / per, within = i - run * per;                  // run = tensor * n_layer + layer
    const bool is_v = run >= n_layer;
    const unsigned layer = is_v ? run - n_layer : run;
    KvBlockPiece p;
    p.cache_off = ((size_t)layer * n_ctx + r0) * E + (size_t)within * 8;
    p.idx = i;
    p.sel = i0 < total ? (is_v ? 2 : 1) : 0;
    p.data = *reinterpret_cast<const uint4 *>(PACK ? (is_v ? vc : kc) + p.cache_off : blk + (size_t)i * 8);
    return p;
}
template <bool PACK>
__device__ __forceinline__ unsigned long long kv_block_store(const KvBlockPiece &p, __half *kc, __half *vc, __half *blk) {
    if (!p.sel) return 0ull;
    *reinterpret_cast<uint4 *>(PACK ? blk + (size_t)p.idx * 8 : (p.sel == 2 ? vc : kc) + p.cache_off) = p.data;
    return (unsigned long long)p.data.x + p.data.y + p.data.z + p.data.w;
}
// PACK: kc / vc are read, blk is written; UNPACK: the reverse.  Not __restrict__ on purpose (above)
template <bool PACK>
__device__ __forceinline__ void kv_block_body(__half *kc, __half *vc, __half *blk, unsigned n_ctx, unsigned n_layer, unsigned E, unsigned r0, unsigned n, unsigned long long *sum) {
    static_assert(KV_COPY_PIECES == 4, "the four pieces are named");
    constexpr int WAVES = KV_COPY_THREADS / 64;
    __shared__ unsigned long long wave_sum[WAVES];
    const unsigned per = n * (E / 8);                                      // 16-byte pieces of one layer's run
    const unsigned total = 2u * n_layer * per;                             // < 2^31 (kv_block_check)
    const unsigned first = blockIdx.x * (KV_COPY_PIECES * KV_COPY_THREADS) + threadIdx.x;
    const KvBlockPiece p0 = kv_block_load<PACK>(kc, vc, blk, first, total, per, n_layer, n_ctx, E, r0);
    const KvBlockPiece p1 = kv_block_load<PACK>(kc, vc, blk, first + KV_COPY_THREADS, total, per, n_layer, n_ctx, E, r0);
    const KvBlockPiece p2 = kv_block_load<PACK>(kc, vc, blk, first + 2 * KV_COPY_THREADS, total, per, n_layer, n_ctx, E, r0);
    const KvBlockPiece p3 = kv_block_load<PACK>(kc, vc, blk, first + 3 * KV_COPY_THREADS, total, per, n_layer, n_ctx, E, r0);
    unsigned long long s = kv_block_store<PACK>(p0, kc, vc, blk);
    s += kv_block_store<PACK>(p1, kc, vc, blk); s += kv_block_store<PACK>(p2, kc, vc, blk); s += kv_block_store<PACK>(p3, kc, vc, blk);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) t += wave_sum[w];
        atomicAdd(sum, t);                                                 // integer sum: order does not matter
    }
}
__global__ __launch_bounds__(KV_COPY_THREADS) void k_kv_pack(const __half *kc, const __half *vc, __half *blk, unsigned n_ctx, unsigned n_layer, unsigned E, unsigned r0, unsigned n,
                                                           unsigned long long *sum) {
    kv_block_body<true>(const_cast<__half *>(kc), const_cast<__half *>(vc), blk, n_ctx, n_layer, E, r0, n, sum);
}
__global__ __launch_bounds__(KV_COPY_THREADS) void k_kv_unpack(const __half *blk, __half *kc, __half *vc, unsigned n_ctx, unsigned n_layer, unsigned E, unsigned r0, unsigned n,
                                                             unsigned long long *sum) {
    kv_block_body<false>(kc, vc, const_cast<__half *>(blk), n_ctx, n_layer, E, r0, n, sum);
}
static unsigned kv_block_check(const char *name, const void *kc, const void *vc, const void *blk, const void *sum, int n_ctx, int n_layer, int E, int r0, int n) {
    static thread_local char msg[96];
    auto bad = [&](const char *what) { snprintf(msg, sizeof(msg), "%s: %s", name, what); throw HipError{hipErrorInvalidValue, msg, __FILE__, __LINE__}; };
    if (!kc || !vc || !blk || !sum || n_layer < 1 || n_ctx < 1 || E < 8 || E % 8 || r0 < 0 || n < 0) bad("bad shape");
    if ((long long)r0 + n > n_ctx) bad("rows outside the cache");
    if ((uintptr_t)kc % 16 || (uintptr_t)vc % 16 || (uintptr_t)blk % 16 || (uintptr_t)sum % 8) bad("a region is not 16-byte aligned");
    const unsigned long long total = 2ull * n_layer * (unsigned long long)n * (E / 8);
    if (total >= (1ull << 31)) bad("2^31 or more pieces");
    return (unsigned)total;
}
void launch_kv_pack(const __half *kc_slot, const __half *vc_slot, int n_ctx, int n_layer, int E, int r0, int n, __half *block, unsigned long long *sum, hipStream_t s) {
    const unsigned total = kv_block_check("launch_kv_pack", kc_slot, vc_slot, block, sum, n_ctx, n_layer, E, r0, n);
    HIP_CHECK(hipMemsetAsync(sum, 0, 8, s));
    if (total == 0) return;
    note_kernel("k_kv_pack");
    const unsigned per_block = KV_COPY_PIECES * KV_COPY_THREADS;
    hipLaunchKernelGGL(k_kv_pack, dim3((total + per_block - 1) / per_block), dim3(KV_COPY_THREADS), 0, s, kc_slot, vc_slot, block, (unsigned)n_ctx, (unsigned)n_layer, (unsigned)E,
                       (unsigned)r0, (unsigned)n, sum);
}
void launch_kv_unpack(const __half *block, __half *kc_slot, __half *vc_slot, int n_ctx, int n_layer, int E, int r0, int n, unsigned long long *sum, hipStream_t s) {
    const unsigned total = kv_block_check("launch_kv_unpack", kc_slot, vc_slot, block, sum, n_ctx, n_layer, E, r0, n);
    HIP_CHECK(hipMemsetAsync(sum, 0, 8, s));
    if (total == 0) return;
    note_kernel("k_kv_unpack");
    const unsigned per_block = KV_COPY_PIECES * KV_COPY_THREADS;
    hipLaunchKernelGGL(k_kv_unpack, dim3((total + per_block - 1) / per_block), dim3(KV_COPY_THREADS), 0, s, block, kc_slot, vc_slot, (unsigned)n_ctx, (unsigned)n_layer, (unsigned)E,
                       (unsigned)r0, (unsigned)n, sum);
}

// =====================================================================================================================
// Beam reordering (Engine::beam_search): conversation slots.s[i] receives rows [r0, r0 + n_rows) of conversation slots.s[parent[i]], every layer, keys and values, for ANY
// map parent -- a swap, a cycle, all-to-one -- in ONE launch, which k_kv_copy (one source, destinations that may not overlap it) cannot express.  Per layer and tensor the
// rows are one contiguous run of n_rows * E halves, cut into 16-byte pieces as in k_kv_copy; ONE thread owns ONE piece position (tensor, layer, row, column piece) in all W
// conversations: it loads the W pieces its conversations are to receive -- piece i from conversation parent[i] -- and only then stores them, skipping i where parent[i] == i.
// No other thread touches any of these 2 W addresses, so no ordering between threads or workgroups is needed whatever the map.  The pointers are not __restrict__ (as in
// k_kv_copy): the loads cannot sink below the stores.  parent comes from device memory (k_beam_select wrote it in this stream); every lane reads the same W words, so the
// identity test and the source choice are uniform (scalar), and an identity map ends every workgroup before it touches the caches.  The slot list travels by value in the
// argument segment (KvPermuteSlots), like KvCopyDst.  The grid follows the piece count.
// The W pieces are NAMED values (PERM_LOAD / PERM_STORE below, `if constexpr` on W), not an indexed array: k_kv_copy's array ended up in LDS.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage), W = 2 | 3 | 4 | 5 | 6 | 7 | 8: 14 | 18 | 22 | 26 | 30 | 34 | 38 VGPRs (4 per piece), 26 | 30 | 34 | 38 | 38 | 46 | 46 SGPRs,
// no scratch, no LDS, occupancy 8 waves per SIMD.
// =====================================================================================================================
constexpr int KV_PERMUTE_THREADS = 256;
__device__ __forceinline__ int kv_permute_slot(const KvPermuteSlots &sl, int j) {   // sl.s[j] for a uniform j without indexing the argument struct
    int v = sl.s[0];
    v = j == 1 ? sl.s[1] : v; v = j == 2 ? sl.s[2] : v; v = j == 3 ? sl.s[3] : v; v = j == 4 ? sl.s[4] : v; v = j == 5 ? sl.s[5] : v; v = j == 6 ? sl.s[6] : v; v = j == 7 ? sl.s[7] : v;
    return v;
}
template <int W>
__global__ __launch_bounds__(KV_PERMUTE_THREADS) void k_kv_permute(__half *kc, __half *vc, size_t seq_stride, const KvPermuteSlots slots, const int *parent, unsigned n_layer,
                                                                  unsigned n_ctx, unsigned E, unsigned r0, unsigned n_rows) {
    static_assert(W >= 2 && W <= KV_PERMUTE_MAX, "beams per search");
    int par[W]; bool identity = true;                                      // uniform: W scalar loads (fully unrolled, constant indices: registers)
#pragma unroll
    for (int i = 0; i < W; i++) { const int p = parent[i]; par[i] = p < 0 || p >= W ? i : p; identity = identity && par[i] == i; }
    if (identity) return;
    const unsigned per = n_rows * (E / 8);                                 // 16-byte pieces of one layer's run
    const unsigned total = 2u * n_layer * per;                             // < 2^31 (launch_kv_permute)
    const unsigned idx = blockIdx.x * KV_PERMUTE_THREADS + threadIdx.x;
    if (idx >= total) return;
    const unsigned run = idx / per, within = idx - run * per;              // run = tensor * n_layer + layer
    const bool is_v = run >= n_layer;
    const unsigned layer = is_v ? run - n_layer : run;
    __half *const base = (is_v ? vc : kc) + ((size_t)layer * n_ctx + r0) * E + (size_t)within * 8;
#define PERM_LOAD(I) uint4 v##I = make_uint4(0u, 0u, 0u, 0u); if constexpr (W > I) { if (par[I] != I) v##I = *reinterpret_cast<const uint4 *>(base + (size_t)kv_permute_slot(slots, par[I]) * seq_stride); }
#define PERM_STORE(I) if constexpr (W > I) { if (par[I] != I) *reinterpret_cast<uint4 *>(base + (size_t)slots.s[I] * seq_stride) = v##I; }
    PERM_LOAD(0) PERM_LOAD(1) PERM_LOAD(2) PERM_LOAD(3) PERM_LOAD(4) PERM_LOAD(5) PERM_LOAD(6) PERM_LOAD(7)
    PERM_STORE(0) PERM_STORE(1) PERM_STORE(2) PERM_STORE(3) PERM_STORE(4) PERM_STORE(5) PERM_STORE(6) PERM_STORE(7)
#undef PERM_LOAD
#undef PERM_STORE
}
void launch_kv_permute(__half *kc, __half *vc, size_t seq_stride, int n_slots, const KvPermuteSlots &slots, int W, const int *parent, int n_layer, int n_ctx, int E, int r0, int r1,
                       hipStream_t s) {
    auto bad = [](const char *what) { throw HipError{hipErrorInvalidValue, what, __FILE__, __LINE__}; };
    if (!kc || !vc || !parent || n_slots < 1 || n_layer < 1 || n_ctx < 1 || E < 8 || E % 8) bad("launch_kv_permute: bad shape");
    if (W < 2 || W > KV_PERMUTE_MAX || W > n_slots) bad("launch_kv_permute: W outside 2 .. 8");
    if (r0 < 0 || r1 < r0 || r1 > n_ctx) bad("launch_kv_permute: rows outside the cache");
    if ((uintptr_t)kc % 16 || (uintptr_t)vc % 16 || seq_stride % 8) bad("launch_kv_permute: a region is not 16-byte aligned");
    if (seq_stride < (size_t)n_layer * n_ctx * E) bad("launch_kv_permute: conversations overlap");
    for (int i = 0; i < W; i++) {
        if (slots.s[i] < 0 || slots.s[i] >= n_slots) bad("launch_kv_permute: slot out of range");
        for (int j = 0; j < i; j++) if (slots.s[j] == slots.s[i]) bad("launch_kv_permute: duplicate slot");
    }
    if (r1 == r0) return;
    const unsigned long long total = 2ull * n_layer * (unsigned long long)(r1 - r0) * (E / 8);
    if (total >= (1ull << 31)) bad("launch_kv_permute: bad shape");
    note_kernel("k_kv_permute<%d>", W);
    const dim3 grid((unsigned)((total + KV_PERMUTE_THREADS - 1) / KV_PERMUTE_THREADS)), block(KV_PERMUTE_THREADS);
#define PERM_CASE(W_) case W_: hipLaunchKernelGGL((k_kv_permute<W_>), grid, block, 0, s, kc, vc, seq_stride, slots, parent, (unsigned)n_layer, (unsigned)n_ctx, (unsigned)E, (unsigned)r0, (unsigned)(r1 - r0)); break
    switch (W) { PERM_CASE(2); PERM_CASE(3); PERM_CASE(4); PERM_CASE(5); PERM_CASE(6); PERM_CASE(7); PERM_CASE(8); }
#undef PERM_CASE
}

// =====================================================================================================================
// Decode attention over the fp16 KV cache: ONE body, attn_llm_body.hpp, included in the kernels k_attn_llm<HD, FUSED, BATCHED, VS> and k_attn_llm_draft<HD, VS> (why
// included and not called: the head of that file); FUSED, BATCHED, DRAFT and VS are compile-time constants there.
// One 512-thread workgroup per (head, query row) -- VS of them with the value-column split below.
//   scores : 16 consecutive lanes share one cached key row (dot16), the new key by one lane over the whole head row (dot_row: sequential fp32 fma over the head dim);
//            q is rounded to fp16 first, like ggml's f16 x f32 mul_mat
//   softmax: max, exp through the fp16 table, exact double sum, probabilities rounded to fp16
//   PV     : thread = (key partition, 8-dim chunk): 16-byte V loads, NPRE in flight; partitions reduced through LDS
// The forms:
//   plain   (!FUSED; prompt rows beyond the prompt kernels' LDS): row t at position *n_past + t, launch_rope_kv has run; every key comes from the cache.
//   FUSED   (decode, one row): RoPE of q / k and the KV append happen in the prologue; the new key / value are also kept in LDS and take the last place of the chains.
//   BATCHED (decode of several conversations in one pass; implies FUSED): row t belongs to conversation row_slot[t], whose position is n_past[row_slot[t]] and whose
//           caches start seq_stride * row_slot[t] elements behind kc / vc.
//   DRAFT   (verify pass, Engine::verify_draft; implies BATCHED): R <= DRAFT_ROWS rows of ONE conversation at the consecutive positions p0 + t, p0 = n_past[row_slot[0]].
//           Row t's keys are the cached rows [0, p0), then this pass's rows 0 .. t - 1, then its own.  No workgroup waits for another: every workgroup rotates and rounds
//           the k / v of rows 0 .. t itself into LDS (at most 8 x HD values; cheaper than a dependency between workgroups) and appends only its own row to the cache.
//           CONTRACT: out and the appended rows are bit for bit those of R launches of the BATCHED form with one row each and n_past advancing by one between them.
// What DRAFT adds to the BATCHED form, and why every fp32 chain keeps its order -- each line below is under `DRAFT`, the rest of the body is shared text:
//   - the position is p0 + t with p0 from row_slot[0]; a row at or past n_ctx returns (the host cuts a draft to the room left: never taken, never a store outside the cache);
//   - the prologue (its own branch) has one thread per (row r <= t, rotated pair) instead of one per pair: rows before t only fill knew / vnew [r], row t is what the
//     BATCHED form does;
//   - the cache is read up to row p0 - 1 only (gmax): rows from p0 on are written by this launch's other workgroups;
//   - a key j in [p0, pos) is taken from LDS (kl / vl) instead of the cache -- SELECTED into the same (partition j mod P, round j / P) place of the same loops, so the
//     max, the score row, and each partition's P.V chain see the same values in the same order (as t < P, a partition holds at most one such key: one LDS read per thread,
//     one select per round); the own key is knew / vnew [t] where the BATCHED form has knew / vnew [0].
// VS in {2, 4} (fused forms only; grid z): the value-column split.  Output dim d of a head is sum_j p_j V[j][d] -- different d never meet -- so VS workgroups share a
// (head, row) with NO hand-off: each computes the whole score row, max, softmax and ph[] (K is read VS times; the splits of a head sit on one XCD's L2) and then the P.V
// chains, the part[] rows and the final sums of ITS HD / VS dims only, on its first AT_THREADS / VS threads = (chunk cv of CH / VS, the same P partitions); the other
// waves skip the V loads and the P.V loops.  Only split 0 appends to the cache; the others read it below pos (DRAFT: below p0), so there is no race.  Every fp32 chain is
// the one of VS == 1 (same keys, same order, same operands): out and the caches are bit-identical.  Per CU the V bytes and P.V instructions fall to 1 / VS.
// =====================================================================================================================
constexpr int AT_THREADS = 512;
// ---- shared by the family (k_attn_llm*, k_attn_split_*, k_attn_ref<true>): operand order and rounding calls are part of the results ----
// the pair (x0, x1) rotated by the angle of (c, s); each kernel rounds the result in its own spelling
__device__ __forceinline__ float2 rope_rot(float x0, float x1, float c, float s) { return make_float2(x0 * c - x1 * s, x0 * s + x1 * c); }
__device__ __forceinline__ __half2 rope_rot_h2(float x0, float x1, float c, float s) { const float2 r = rope_rot(x0, x1, c, s); return __floats2half2_rn(r.x, r.y); }
__device__ __forceinline__ void st_h2(__half *p, __half2 v) { *reinterpret_cast<__half2 *>(p) = v; }
// the eight halves of a 16-byte piece as floats, in element order
__device__ __forceinline__ void unpack8(const int4 &v, float (&f)[8]) {
    const unsigned w[4] = {(unsigned)v.x, (unsigned)v.y, (unsigned)v.z, (unsigned)v.w};
#pragma unroll
    for (int e = 0; e < 4; e++) { f[2 * e] = h2f_bits(w[e] & 0xFFFF); f[2 * e + 1] = h2f_bits(w[e] >> 16); }
}
// score of one key whose row is spread over CH consecutive lanes (lane c: dims 8 c .. 8 c + 7 in kk, the same dims of q in qd): all CH lanes return it
template <int CH> __device__ __forceinline__ float dot16(const int4 &kk, const float (&qd)[8], float scale) {
    float kf[8], s = 0.0f;
    unpack8(kk, kf);
#pragma unroll
    for (int e = 0; e < 8; e++) s = fmaf(kf[e], qd[e], s);
    s += dpp_f<0xB1>(s); s += dpp_f<0x4E>(s);                     // the CH = HD / 8 lanes of the key: 4 (HD 32), 8 (HD 64: half a DPP row) or 16 (HD 128: a DPP row)
    if (CH >= 8) s += dpp_f<0x141>(s);
    if (CH >= 16) s += dpp_f<0x140>(s);
    return s * scale;
}
__device__ __forceinline__ void pv_acc(float (&o)[8], const int4 &vv, float pj) {   // o += pj * (the eight values of vv)
    const unsigned w[4] = {(unsigned)vv.x, (unsigned)vv.y, (unsigned)vv.z, (unsigned)vv.w};
#pragma unroll
    for (int e = 0; e < 4; e++) { o[2 * e] = fmaf(h2f_bits(w[e] & 0xFFFF), pj, o[2 * e]); o[2 * e + 1] = fmaf(h2f_bits(w[e] >> 16), pj, o[2 * e + 1]); }
}
// Dynamic LDS of the body for contexts up to n_ctx with `rows` new rows kept in LDS (1, or DRAFT_ROWS for the DRAFT form) -- the ONLY place the layout's size is
// written: sc [Tpad] fp32 | ph [Tpad] | qh [hd] | knew [rows][hd] | vnew [rows][hd] | part [P][hd] fp32 | 64 spare
static size_t attn_lds_bytes(int n_ctx, int hd, int rows) {
    const int Tpad = (n_ctx + 7) & ~7;
    return (size_t)Tpad * 6 + (size_t)hd * 2 + (size_t)2 * rows * hd * 2 + (size_t)(AT_THREADS / (hd / 8)) * hd * 4 + 64;
}
static int attn_ctx_that_fits(int hd, int rows) { int n = 0; while (attn_lds_bytes(n + 8, hd, rows) + 256 /* static reduction arrays */ <= 160 * 1024) n += 8; return n; }
int attn_max_ctx(int hd) { return attn_ctx_that_fits(hd, 1); }
int attn_draft_max_ctx(int hd) { return attn_ctx_that_fits(hd, DRAFT_ROWS); }

// Argument order (see "Kernel arguments" above matvec_run): what the prologue's first loads need -- the position's address, the three projections, the two RoPE tables
// and E, 13 dwords -- stands in front, inside the preloaded head; the caches, the exp table and the output follow.  The position itself lives in device memory, so its load
// stays: MG4_ATTN_PIN (in the body, right behind that load) consumes the position and every argument, so all of them are requested in the position's round trip and none
// in a further one behind it.
#define MG4_ATTN_PIN() asm volatile("" ::"s"(pos_), "s"(q), "s"(kin), "s"(vin), "s"(cos_tab), "s"(sin_tab), "s"(E), "s"(kc), "s"(vc), "s"(tb.exp), "s"(out))
template <int HD, bool FUSED, bool BATCHED = false, int VS = 1>
__global__ __launch_bounds__(AT_THREADS) void k_attn_llm(const int *__restrict__ n_past, float *__restrict__ q, const float *__restrict__ kin, const float *__restrict__ vin,
                                                         const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, int E, __half *__restrict__ kc,
                                                         __half *__restrict__ vc, const Tables tb, float *__restrict__ out, const int *__restrict__ row_slot = nullptr,
                                                         size_t seq_stride = 0) {
    constexpr bool DRAFT = false;
    constexpr int n_ctx = 0;                                      // DRAFT only
#include "attn_llm_body.hpp"
}
template <int HD, int VS = 1>
__global__ __launch_bounds__(AT_THREADS) void k_attn_llm_draft(const int *__restrict__ n_past, float *__restrict__ q, const float *__restrict__ kin, const float *__restrict__ vin,
                                                               const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, int E, int n_ctx, __half *__restrict__ kc,
                                                               __half *__restrict__ vc, const Tables tb, float *__restrict__ out, const int *__restrict__ row_slot,
                                                               size_t seq_stride) {
    constexpr bool FUSED = true, BATCHED = true, DRAFT = true;
#include "attn_llm_body.hpp"
}
#undef MG4_ATTN_PIN
// MDRAFT (verify pass of SEVERAL conversations, Engine::verify_draft_batch): the N <= 64 rows of the pass are consecutive groups, group g = R_g <= DRAFT_ROWS rows of
// conversation slot_g at the positions p0_g + 0 .. R_g - 1, p0_g = n_past[slot_g] (k_mdraft_begin has written it), all slots distinct.  Row t knows its conversation
// row_slot[t] and its position row_pos[t]: its index inside the group is r = row_pos[t] - p0 and the group's first packed row is t - r -- no table of groups.  Everything
// else is the DRAFT form with (t - r, r) where DRAFT has (0, t): row t rotates and rounds the k / v of the packed rows t - r .. t into LDS, appends only its own, reads
// the cache below p0 only and SELECTS a key in [p0, pos) from LDS into the same (partition j mod P, round j / P) place of the same loops; no workgroup waits for another.
// CONTRACT: out and the appended rows are bit for bit those of one launch_attn_llm_draft per group.
// Its own body text and not a further constant of attn_llm_body.hpp: the twelve k_attn_llm and the k_attn_llm_draft instantiations stay the validated ISA untouched
// (tools/isa_diff.py).  The statements below are that file's DRAFT lines, in its order, with the same helpers: operand order and rounding calls are part of the results.
// Arguments: the two row arrays and the positions' address lead (the position is two dependent loads away: row_slot[t], then n_past[slot]), the projections, the RoPE
// tables and E follow inside the preloadable head; one empty asm consumes every argument in the first round trip, as MG4_ATTN_PIN does for the other forms.
// A row whose (slot, position) does not describe a place inside a group (r outside [0, min(t, DRAFT_ROWS - 1)]) or that lies at or past n_ctx returns without a store.
template <int HD, int VS = 1>
__global__ __launch_bounds__(AT_THREADS) void k_attn_llm_mdraft(const int *__restrict__ row_slot, const int *__restrict__ row_pos, const int *__restrict__ n_past, float *__restrict__ q,
                                                                const float *__restrict__ kin, const float *__restrict__ vin, const float *__restrict__ cos_tab,
                                                                const float *__restrict__ sin_tab, int E, int n_ctx, __half *__restrict__ kc, __half *__restrict__ vc, const Tables tb,
                                                                float *__restrict__ out, size_t seq_stride) {
    static_assert(VS == 1 || ((VS == 2 || VS == 4) && (HD / 8) % VS == 0), "the value-column split: 2 or 4 workgroups per (head, row)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int CH = HD / 8, P = AT_THREADS / CH, RM = DRAFT_ROWS;
    static_assert(RM <= P && RM * (HD / 2) <= AT_THREADS, "one prologue thread per (row, rotated pair); at most one LDS key per partition");
    const int h = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    constexpr int CHV = (HD / 8) / VS;
    const bool vact = VS == 1 || tid < AT_THREADS / VS;
    const int slot = row_slot[t], pos = row_pos[t];
    asm volatile("" ::"s"(slot), "s"(pos), "s"(n_past), "s"(q), "s"(kin), "s"(vin), "s"(cos_tab), "s"(sin_tab), "s"(E), "s"(kc), "s"(vc), "s"(tb.exp), "s"(out));
    const int p0 = n_past[slot], r = pos - p0, t0 = t - r;          // the group's first position, this row's index in the group, the group's first packed row
    if (r < 0 || r >= RM || r > t || pos >= n_ctx) return;
    kc += (size_t)slot * seq_stride; vc += (size_t)slot * seq_stride;
    const int T = pos + 1, Tg = pos;                               // Tg: keys that are not this row's own
    const int Tpad = (T + 7) & ~7;
    float *sc = reinterpret_cast<float *>(smem);                  // [Tpad]                 (the carve-up attn_lds_bytes sizes)
    __half *ph = reinterpret_cast<__half *>(sc + Tpad);           // [Tpad]
    __half *qh = ph + Tpad;                                       // [HD]
    __half *knew = qh + HD, *vnew = knew + RM * HD;               // [RM][HD] each: rows 0 .. r of the group
    float *part = reinterpret_cast<float *>(vnew + RM * HD);      // [P][HD]
    __shared__ float s_red[AT_THREADS / 64];
    __shared__ double s_dred[AT_THREADS / 64];
    const float scale = 1.0f / sqrtf((float)HD);
    const size_t qo = (size_t)t * E + (size_t)h * HD;
    if (tid < (r + 1) * (HD / 2)) {                               // one thread per (row rr <= r of the group, rotated pair): rows before r only fill knew / vnew [rr]
        const int rr = tid / (HD / 2), i = tid % (HD / 2), pr = p0 + rr;
        const size_t ro = (size_t)(t0 + rr) * E + (size_t)h * HD;
        const float c = cos_tab[(size_t)pr * (HD / 2) + i], s = sin_tab[(size_t)pr * (HD / 2) + i];
        const __half2 kr = rope_rot_h2(kin[ro + 2 * i], kin[ro + 2 * i + 1], c, s);
        const __half2 vr = __floats2half2_rn(vin[ro + 2 * i], vin[ro + 2 * i + 1]);
        st_h2(knew + rr * HD + 2 * i, kr); st_h2(vnew + rr * HD + 2 * i, vr);
        if (rr == r) {
            st_h2(qh + 2 * i, rope_rot_h2(q[qo + 2 * i], q[qo + 2 * i + 1], c, s));
            const size_t co = (size_t)pos * E + (size_t)h * HD + 2 * i;
            if (VS == 1 || blockIdx.z == 0) { st_h2(kc + co, kr); st_h2(vc + co, vr); }
        }
    }
    __syncthreads();
    unsigned qreg[HD / 2];
#pragma unroll
    for (int i = 0; i < HD / 8; i++) { const int4 v4 = *reinterpret_cast<const int4 *>(qh + 8 * i); qreg[4 * i] = (unsigned)v4.x; qreg[4 * i + 1] = (unsigned)v4.y; qreg[4 * i + 2] = (unsigned)v4.z; qreg[4 * i + 3] = (unsigned)v4.w; }
    auto dot_row = [&](const __half *kr) {
        int4 kk[HD / 8];
#pragma unroll
        for (int i = 0; i < HD / 8; i++) kk[i] = ld16(kr + 8 * i);
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < HD / 8; i++) {
            const unsigned w[4] = {(unsigned)kk[i].x, (unsigned)kk[i].y, (unsigned)kk[i].z, (unsigned)kk[i].w};
#pragma unroll
            for (int e = 0; e < 4; e++) { s = fmaf(h2f_bits(w[e] & 0xFFFF), h2f_bits(qreg[4 * i + e] & 0xFFFF), s); s = fmaf(h2f_bits(w[e] >> 16), h2f_bits(qreg[4 * i + e] >> 16), s); }
        }
        return s * scale;
    };
    const int c = tid % CH, p = tid / CH;
    const int cv = VS == 1 ? c : (int)blockIdx.z * CHV + tid % CHV, pv = VS == 1 ? p : tid / CHV;
    const __half *kb = kc + (size_t)h * HD + 8 * c, *vb = vc + (size_t)h * HD + 8 * cv;
    constexpr int NPRE = 16;
    const int gmax = max(p0 - 1, 0);                              // the last row the cache is read at: rows from p0 on are written by this launch (loads are clamped, never a branch)
    int4 kpre[NPRE], vpre[NPRE];
#pragma unroll
    for (int i = 0; i < NPRE; i++) kpre[i] = ld16(kb + (size_t)min(p + i * P, gmax) * E);
    if (vact) {
#pragma unroll
        for (int i = 0; i < NPRE; i++) vpre[i] = ld16(vb + (size_t)min(pv + i * P, gmax) * E);
    }
    // this partition's key among the group's earlier rows, if any: row rl at position jl (jl mod P == p)
    const int rl = (p - p0) & (P - 1), rlv = (pv - p0) & (P - 1);
    const int jl = rl < r ? p0 + rl : -1, jlv = rlv < r ? p0 + rlv : -1;
    const int4 kl = *reinterpret_cast<const int4 *>(knew + min(rl, RM - 1) * HD + 8 * c), vl = *reinterpret_cast<const int4 *>(vnew + min(rlv, RM - 1) * HD + 8 * cv);
    float qd[8];
    unpack8(*reinterpret_cast<const int4 *>(qh + 8 * c), qd);
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NPRE; i++) { const int j = p + i * P; const float s = dot16<CH>(j == jl ? kl : kpre[i], qd, scale); if (j < Tg) { if (c == 0) sc[j] = s; mx = fmaxf(mx, s); } }
    for (int j0 = p + NPRE * P; j0 < Tg; j0 += 8 * P) {          // beyond the prefetch: 8 rows per round trip
        int4 kk[8];
#pragma unroll
        for (int i = 0; i < 8; i++) kk[i] = ld16(kb + (size_t)min(j0 + i * P, gmax) * E);
#pragma unroll
        for (int i = 0; i < 8; i++) { const int j = j0 + i * P; const float s = dot16<CH>(j == jl ? kl : kk[i], qd, scale); if (j < Tg) { if (c == 0) sc[j] = s; mx = fmaxf(mx, s); } }
    }
    if (tid == AT_THREADS - 1) { const float s = dot_row(knew + r * HD); sc[pos] = s; mx = fmaxf(mx, s); }
    mx = wave_max(mx);
    if ((tid & 63) == 0) s_red[tid >> 6] = mx;
    __syncthreads();
    mx = s_red[0];
#pragma unroll
    for (int i = 1; i < AT_THREADS / 64; i++) mx = fmaxf(mx, s_red[i]);
    double sum = 0.0;
    for (int j = tid; j < T; j += AT_THREADS) { const float v = exp_h(tb.exp, sc[j] - mx); sc[j] = v; sum += (double)v; }
    sum = wave_sum_d(sum);
    if ((tid & 63) == 0) s_dred[tid >> 6] = sum;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < AT_THREADS / 64; i++) tot += s_dred[i];
    const float inv = (float)(1.0 / tot);
    for (int j = tid; j < T; j += AT_THREADS) ph[j] = f2h_rn(sc[j] * inv);
    __syncthreads();
    float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto pv_key = [&](const int4 &vv, const int j) { pv_acc(o, vv, __half2float(ph[j])); };
    if (vact) {                                                   // VS > 1: the other waves skip (wave-uniform; no barrier inside)
#pragma unroll
        for (int i = 0; i < NPRE; i++) { const int j = pv + i * P; if (j < Tg) pv_key(j == jlv ? vl : vpre[i], j); }
        for (int j0 = pv + NPRE * P; j0 < Tg; j0 += 8 * P) {
            int4 vv[8];
#pragma unroll
            for (int i = 0; i < 8; i++) vv[i] = ld16(vb + (size_t)min(j0 + i * P, gmax) * E);
#pragma unroll
            for (int i = 0; i < 8; i++) { const int j = j0 + i * P; if (j < Tg) pv_key(j == jlv ? vl : vv[i], j); }
        }
        if (pv == P - 1) {
            const float pj = __half2float(ph[pos]);
#pragma unroll
            for (int e = 0; e < 8; e++) o[e] = fmaf(__half2float(vnew[r * HD + 8 * cv + e]), pj, o[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; e++) part[pv * HD + 8 * cv + e] = o[e];
    }
    __syncthreads();
    // the partitions in order 0 .. P - 1, as ever; VS > 1: this workgroup's HD / VS dims
    for (int i = (VS == 1 ? 0 : (int)blockIdx.z * (HD / VS)) + tid; i < (VS == 1 ? HD : ((int)blockIdx.z + 1) * (HD / VS)); i += AT_THREADS) { float s = 0.0f;
#pragma unroll 8
        for (int pp = 0; pp < P; pp++) s += part[pp * HD + i];
        out[qo + i] = s; }
}

// the supported head sizes as compile-time constants: f(std::integral_constant<int, HD>) for hd's HD; false (f not called) for an unsupported head size
template <class F> static bool attn_for_head_size(int hd, F &&f) {
    switch (hd) {
    case 32: f(std::integral_constant<int, 32>{}); return true;
    case 64: f(std::integral_constant<int, 64>{}); return true;
    case 128: f(std::integral_constant<int, 128>{}); return true;
    default: return false;
    }
}
// the decode launchers' answer to an unsupported head size (the prompt launchers return false instead)
template <class F> static void attn_for_head_size_or_throw(int hd, F &&f) {
    if (!attn_for_head_size(hd, f)) throw HipError{hipErrorInvalidValue, "unsupported head size", __FILE__, __LINE__};
}
// The one launcher of the body's kernels: grid (head, row, value-column split), the layout's LDS, the > 64 KiB opt-in at the first launch of every instantiation (the
// plain and the one-row fused form together, as they always were).  z is the split: with 40 or 32 heads the workgroups h + n_head (t + rows z) of a head's splits land on
// the same XCD and share its L2 for the K rows they all read.
template <int HD, bool BATCHED, bool DRAFT, int VS>
static void launch_attn_body_vs(bool fused, float *q, const float *k, const float *v, __half *kc, __half *vc, int rows, int n_head, const int *n_past, const int *row_slot,
                                size_t seq_stride, int n_ctx, const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, hipStream_t s) {
    const size_t lds = attn_lds_bytes(n_ctx, HD, DRAFT ? DRAFT_ROWS : 1);
    const dim3 grid((unsigned)n_head, (unsigned)rows, (unsigned)VS);
    static bool attr = false;
    if constexpr (DRAFT) {
        if (!attr) { HIP_IGNORE(lds_optin_max(&k_attn_llm_draft<HD, VS>)); attr = true; }
        if (VS == 1) note_kernel("k_attn_llm_draft<%d>", HD); else note_kernel("k_attn_llm_draft<%d, %d>", HD, VS);
        hipLaunchKernelGGL((k_attn_llm_draft<HD, VS>), grid, dim3(AT_THREADS), lds, s, n_past, q, k, v, cos_tab, sin_tab, n_head * HD, n_ctx, kc, vc, tb, out, row_slot, seq_stride);
    } else if constexpr (BATCHED) {
        if (!attr) { HIP_IGNORE(lds_optin_max(&k_attn_llm<HD, true, true, VS>)); attr = true; }
        hipLaunchKernelGGL((k_attn_llm<HD, true, true, VS>), grid, dim3(AT_THREADS), lds, s, n_past, q, k, v, cos_tab, sin_tab, n_head * HD, kc, vc, tb, out, row_slot, seq_stride);
    } else if constexpr (VS == 1) {
        if (!attr) { HIP_IGNORE(lds_optin_max(&k_attn_llm<HD, true>));
                     HIP_IGNORE(lds_optin_max(&k_attn_llm<HD, false>)); attr = true; }
        note_kernel("k_attn_llm<%d, %s, false>", HD, fused ? "true" : "false");
        hipLaunchKernelGGL((fused ? k_attn_llm<HD, true> : k_attn_llm<HD, false>), grid, dim3(AT_THREADS), lds, s, n_past, q, k, v, cos_tab, sin_tab, n_head * HD, kc, vc, tb, out,
                           row_slot, seq_stride);
    } else {
        if (!attr) { HIP_IGNORE(lds_optin_max(&k_attn_llm<HD, true, false, VS>)); attr = true; }
        note_kernel("k_attn_llm<%d, true, false, %d>", HD, VS);
        hipLaunchKernelGGL((k_attn_llm<HD, true, false, VS>), grid, dim3(AT_THREADS), lds, s, n_past, q, k, v, cos_tab, sin_tab, n_head * HD, kc, vc, tb, out, row_slot, seq_stride);
    }
}
// vs: 1, or 2 / 4 for the fused forms where the head's HD / 8 chunks divide (every supported head size does); anything else is refused
bool attn_vsplit_ok(int hd, int vs) { return vs == 1 || ((vs == 2 || vs == 4) && (hd == 32 || hd == 64 || hd == 128)); }
template <int HD, bool BATCHED, bool DRAFT>
static void launch_attn_body(bool fused, float *q, const float *k, const float *v, __half *kc, __half *vc, int rows, int n_head, const int *n_past, const int *row_slot,
                             size_t seq_stride, int n_ctx, const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, int vs, hipStream_t s) {
    if (!attn_vsplit_ok(HD, vs) || (vs != 1 && !fused)) throw HipError{hipErrorInvalidValue, "decode attention: unsupported value-column split", __FILE__, __LINE__};
#define ATTN_VS_ARGS fused, q, k, v, kc, vc, rows, n_head, n_past, row_slot, seq_stride, n_ctx, cos_tab, sin_tab, tb, out, s
    if (vs == 4) launch_attn_body_vs<HD, BATCHED, DRAFT, 4>(ATTN_VS_ARGS);
    else if (vs == 2) launch_attn_body_vs<HD, BATCHED, DRAFT, 2>(ATTN_VS_ARGS);
    else launch_attn_body_vs<HD, BATCHED, DRAFT, 1>(ATTN_VS_ARGS);
#undef ATTN_VS_ARGS
}
// fused = true (N must be 1): q,k,v are the raw projections; RoPE + KV append happen inside.  fused = false: launch_rope_kv must have run.
void launch_attn_llm(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int N, int n_head, int hd, const int *n_past, int n_ctx,
                     const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, bool fused, hipStream_t s, int vs) {
    attn_for_head_size_or_throw(hd, [&](auto tag) {
        launch_attn_body<decltype(tag)::value, false, false>(fused, q, k, v, kcache, vcache, fused ? 1 : N, n_head, n_past, nullptr, 0, n_ctx, cos_tab, sin_tab, tb, out, vs, s); });
}
// Decode attention for B rows of B different conversations (RoPE + KV append fused): row t uses position n_past[row_slot[t]] and the caches of that conversation.
void launch_attn_llm_batched(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int B, int n_head, int hd, const int *n_past, const int *row_slot,
                             size_t seq_stride, int n_ctx, const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, hipStream_t s, int vs) {
    attn_for_head_size_or_throw(hd, [&](auto tag) {
        launch_attn_body<decltype(tag)::value, true, false>(true, q, k, v, kcache, vcache, B, n_head, n_past, row_slot, seq_stride, n_ctx, cos_tab, sin_tab, tb, out, vs, s); });
}
// Verify pass: R <= DRAFT_ROWS rows of the conversation row_slot[0] (the DRAFT form above); n_ctx <= attn_draft_max_ctx(hd)
void launch_attn_llm_draft(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int R, int n_head, int hd, const int *n_past, const int *row_slot,
                           size_t seq_stride, int n_ctx, const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, hipStream_t s, int vs) {
    if (R < 1 || R > DRAFT_ROWS) throw HipError{hipErrorInvalidValue, "launch_attn_llm_draft: row count out of range", __FILE__, __LINE__};
    attn_for_head_size_or_throw(hd, [&](auto tag) {
        launch_attn_body<decltype(tag)::value, true, true>(true, q, k, v, kcache, vcache, R, n_head, n_past, row_slot, seq_stride, n_ctx, cos_tab, sin_tab, tb, out, vs, s); });
}
// Verify pass of several conversations: N <= ATTN_MDRAFT_ROWS packed rows in groups (k_attn_llm_mdraft above); n_ctx <= attn_draft_max_ctx(hd)
template <int HD, int VS>
static void launch_attn_mdraft_vs(float *q, const float *k, const float *v, __half *kc, __half *vc, int N, int n_head, const int *n_past, const int *row_slot, const int *row_pos,
                                  size_t seq_stride, int n_ctx, const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, hipStream_t s) {
    static bool attr = false;
    if (!attr) { HIP_IGNORE(lds_optin_max(&k_attn_llm_mdraft<HD, VS>)); attr = true; }
    if (VS == 1) note_kernel("k_attn_llm_mdraft<%d>", HD); else note_kernel("k_attn_llm_mdraft<%d, %d>", HD, VS);
    hipLaunchKernelGGL((k_attn_llm_mdraft<HD, VS>), dim3((unsigned)n_head, (unsigned)N, (unsigned)VS), dim3(AT_THREADS), attn_lds_bytes(n_ctx, HD, DRAFT_ROWS), s, row_slot, row_pos, n_past, q,
                       k, v, cos_tab, sin_tab, n_head * HD, n_ctx, kc, vc, tb, out, seq_stride);
}
void launch_attn_llm_draft_batched(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int N, int n_head, int hd, const int *n_past, const int *row_slot,
                                   const int *row_pos, size_t seq_stride, int n_ctx, const float *cos_tab, const float *sin_tab, const Tables &tb, float *out, hipStream_t s, int vs) {
    if (N < 1 || N > ATTN_MDRAFT_ROWS) throw HipError{hipErrorInvalidValue, "launch_attn_llm_draft_batched: row count out of range", __FILE__, __LINE__};
    if (n_ctx < 1 || n_ctx > attn_draft_max_ctx(hd)) throw HipError{hipErrorInvalidValue, "launch_attn_llm_draft_batched: n_ctx beyond what the verify form holds in LDS", __FILE__, __LINE__};
    attn_for_head_size_or_throw(hd, [&](auto tag) {
        constexpr int HD = decltype(tag)::value;
        if (!attn_vsplit_ok(HD, vs)) throw HipError{hipErrorInvalidValue, "decode attention: unsupported value-column split", __FILE__, __LINE__};
#define ATTN_MD_ARGS q, k, v, kcache, vcache, N, n_head, n_past, row_slot, row_pos, seq_stride, n_ctx, cos_tab, sin_tab, tb, out, s
        if (vs == 4) launch_attn_mdraft_vs<HD, 4>(ATTN_MD_ARGS);
        else if (vs == 2) launch_attn_mdraft_vs<HD, 2>(ATTN_MD_ARGS);
        else launch_attn_mdraft_vs<HD, 1>(ATTN_MD_ARGS);
#undef ATTN_MD_ARGS
    });
}
// =====================================================================================================================
// Key-split decode attention (long contexts): k_attn_llm above puts ONE workgroup on a head -- 40 workgroups on a 256-CU chip, 0.015 us per cached key, 35 us per layer
// at 2048 keys.  Here S workgroups share a head's keys (n_head x S >= 240 workgroups) in two launches; nothing spins, so nothing can hang:
//   k_attn_split_scores : (head, split) -> RoPE of q / k (every workgroup; split 0 appends k, v to the cache), scores of its key range into a per-head fp32 row in HBM
//                         (16 lanes per 256-byte key row, DPP reduction -- the arithmetic of k_attn_llm), the new key's score by the last split;
//   k_attn_split_pv     : (head, split) -> every workgroup reads the head's whole score row (T x 4 bytes), max, fp16-table exp, exact sum, 1 / sum (identical in all S
//                         workgroups: the same values in, order-independent exact arithmetic); probabilities rounded to fp16 and P.V over ITS key range; the partial
//                         output goes out as device-scope (sc1) stores, an arrival counter per head names the last workgroup, and that one adds the S partials in
//                         split order (deterministic) and resets the counter for the next launch.
// Softmax semantics are those of k_attn_llm (global max BEFORE the table lookups: the fp16 exp table does not allow the flash-decoding rescale).
// =====================================================================================================================
constexpr int AS_THREADS = 256;
template <int HD>
__global__ __launch_bounds__(AS_THREADS) void k_attn_split_scores(const float *__restrict__ q, const float *__restrict__ kin, const float *__restrict__ vin, __half *__restrict__ kc,
                                                                   __half *__restrict__ vc, int E, const int *__restrict__ n_past, const float *__restrict__ cos_tab,
                                                                   const float *__restrict__ sin_tab, float *__restrict__ scores, int ld_scores, __half *__restrict__ qrot) {
    constexpr int CH = HD / 8, P = AS_THREADS / CH;
    constexpr int NR = 16;                                        // key rows per lane group in flight (16 x P x 256 B = 64 KiB per workgroup at HD 128)
    const int h = blockIdx.x, sp = blockIdx.y, S = gridDim.y, tid = threadIdx.x;
    const int pos = *n_past, Tg = pos;                            // keys 0 .. pos - 1 come from the cache, key pos is this step's
    __shared__ __attribute__((aligned(16))) __half qh[HD];
    __shared__ __attribute__((aligned(16))) __half knew[HD];
    const float scale = 1.0f / sqrtf((float)HD);
    const size_t qo = (size_t)h * HD;
    const int c = tid % CH, p = tid / CH;
    const int per = ((Tg + S - 1) / S + P - 1) / P * P;           // keys per split, a whole number of passes
    const int j_lo = sp * per, j_hi = min(Tg, j_lo + per), j_cl = max(j_hi - 1, 0);
    const __half *kb = kc + (size_t)h * HD + 8 * c;
    // the first NR key rows of this lane group do not depend on q: requested before the RoPE prologue and its barrier
    int4 kk[NR];
#pragma unroll
    for (int i = 0; i < NR; i++) kk[i] = ld16(kb + (size_t)min(j_lo + p + i * P, j_cl) * E);
    if (tid < HD / 2) {
        const int i = tid;
        const float cs = cos_tab[(size_t)pos * (HD / 2) + i], sn = sin_tab[(size_t)pos * (HD / 2) + i];
        const float2 qf = rope_rot(q[qo + 2 * i], q[qo + 2 * i + 1], cs, sn), kf = rope_rot(kin[qo + 2 * i], kin[qo + 2 * i + 1], cs, sn);
        const __half2 qr = __halves2half2(f2h_rn(qf.x), f2h_rn(qf.y)), kr = __halves2half2(f2h_rn(kf.x), f2h_rn(kf.y));
        st_h2(qh + 2 * i, qr); st_h2(knew + 2 * i, kr);
        if (sp == 0) {
            const __half2 vr = __halves2half2(f2h_rn(vin[qo + 2 * i]), f2h_rn(vin[qo + 2 * i + 1]));
            const size_t co = (size_t)pos * E + (size_t)h * HD + 2 * i;
            st_h2(kc + co, kr); st_h2(vc + co, vr);
            st_h2(qrot + qo + 2 * i, qr);                           // (diagnostics / tests)
        }
    }
    __syncthreads();
    float qd[8];
    unpack8(*reinterpret_cast<const int4 *>(qh + 8 * c), qd);
    float *srow = scores + (size_t)h * ld_scores;
    for (int j0 = j_lo + p; j0 < j_hi; j0 += NR * P) {
        int4 nx[NR];
        const bool more = j0 + NR * P < j_hi;                     // wave-uniform up to the lane group; clamped loads keep it branch-free
#pragma unroll
        for (int i = 0; i < NR; i++) nx[i] = ld16(kb + (size_t)min(j0 + (NR + i) * P, j_cl) * E);
#pragma unroll
        for (int i = 0; i < NR; i++) { const int j = j0 + i * P; const float s = dot16<CH>(kk[i], qd, scale); if (j < j_hi && c == 0) srow[j] = s; }
        (void)more;
#pragma unroll
        for (int i = 0; i < NR; i++) kk[i] = nx[i];
    }
    if (sp == S - 1 && tid == 0) {                                // this step's key: one lane, the whole row in element order (k_attn_llm's dot_row)
        float s = 0.0f;
        for (int i = 0; i < HD; i++) s = fmaf(__half2float(knew[i]), __half2float(qh[i]), s);
        srow[pos] = s * scale;
    }
}
template <int HD>
__global__ __launch_bounds__(AS_THREADS) void k_attn_split_pv(const float *__restrict__ scores, int ld_scores, const __half *__restrict__ vc, int E, const int *__restrict__ n_past,
                                                               const Tables tb, float *__restrict__ partial, unsigned *__restrict__ arrive, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_sp[];
    constexpr int CH = HD / 8, P = AS_THREADS / CH;
    const int h = blockIdx.x, sp = blockIdx.y, S = gridDim.y, tid = threadIdx.x;
    const int pos = *n_past, T = pos + 1;
    float *sc = reinterpret_cast<float *>(smem_sp);               // [T] scores, then exp values
    float *part = sc + ((T + 3) & ~3);                            // [P][HD]
    __shared__ float s_red[AS_THREADS / 64];
    __shared__ double s_dred[AS_THREADS / 64];
    __shared__ int s_last;
    constexpr int NR = 16;
    // this split's key range of the T keys (key pos included: it was appended by the score launch); its first NR value rows do not depend on the softmax: requested first
    const int per = ((T + S - 1) / S + P - 1) / P * P;
    const int j_lo = sp * per, j_hi = min(T, j_lo + per), j_cl = max(j_hi - 1, 0);
    const int c = tid % CH, p = tid / CH;
    const __half *vb = vc + (size_t)h * HD + 8 * c;
    int4 vv[NR];
#pragma unroll
    for (int i = 0; i < NR; i++) vv[i] = ld16(vb + (size_t)min(j_lo + p + i * P, j_cl) * E);
    const float *srow = scores + (size_t)h * ld_scores;
    float mx = -INFINITY;
    for (int j = tid; j < T; j += AS_THREADS) { const float s = srow[j]; sc[j] = s; mx = fmaxf(mx, s); }
    mx = wave_max(mx);
    if ((tid & 63) == 0) s_red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    double sum = 0.0;
    for (int j0 = tid; j0 < T; j0 += 4 * AS_THREADS) {            // four independent table gathers in flight per thread
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int j = j0 + u * AS_THREADS; v[u] = j < T ? exp_h(tb.exp, sc[j] - mx) : 0.0f; }
#pragma unroll
        for (int u = 0; u < 4; u++) { const int j = j0 + u * AS_THREADS; if (j < T) { sc[j] = v[u]; sum += (double)v[u]; } }   // fp16 values: the double sum is exact in any order
    }
    sum = wave_sum_d(sum);
    if ((tid & 63) == 0) s_dred[tid >> 6] = sum;
    __syncthreads();
    const float inv = (float)(1.0 / (((s_dred[0] + s_dred[1]) + s_dred[2]) + s_dred[3]));
    float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j0 = j_lo + p; j0 < j_hi; j0 += NR * P) {
        int4 nx[NR];
#pragma unroll
        for (int i = 0; i < NR; i++) nx[i] = ld16(vb + (size_t)min(j0 + (NR + i) * P, j_cl) * E);
#pragma unroll
        for (int i = 0; i < NR; i++) {
            const int j = j0 + i * P;
            if (j < j_hi) pv_acc(o, vv[i], __half2float(f2h_rn(sc[j] * inv)));
        }
#pragma unroll
        for (int i = 0; i < NR; i++) vv[i] = nx[i];
    }
#pragma unroll
    for (int e = 0; e < 8; e++) part[p * HD + 8 * c + e] = o[e];
    __syncthreads();
    float *mine = partial + ((size_t)h * S + sp) * HD;
    for (int i = tid; i < HD; i += AS_THREADS) {
        float s = 0.0f;
#pragma unroll 8
        for (int pp = 0; pp < P; pp++) s += part[pp * HD + i];
        __hip_atomic_store(mine + i, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // device-scope (sc1) store: visible to a reader on another XCD without a cache flush
    }
    // Hand-off form (cdna_hip_programming.md Guideline 16, R1; MI355X_MICROARCH.md "Valid forms"): payload by write-through (sc1) stores, EVERY storing thread drains
    // vmcnt(0), workgroup barrier, ONE lane's agent-scope arrival; the reader (below) takes the payload with sc1 loads, which the guide lists as replacing the acquire when
    // the producer stored sc1.  A release on the arrival would add buffer_wbl2 (~1.7 us) to every one of the n_head x S workgroups of every layer.  Exercised across XCDs
    // at the real head count by tests/test_gpu_parity.py::test_key_split_attention_at_the_13b_head_count_is_bit_identical.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // this thread's partial stores have completed ...
    __syncthreads();                                              // ... and so have everybody's, before the arrival is counted
    if (tid == 0) s_last = __hip_atomic_fetch_add(arrive + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(S - 1);
    __syncthreads();
    if (!s_last) return;
    for (int i = tid; i < HD; i += AS_THREADS) {                  // the last workgroup of the head: the S partials in split order
        float s = 0.0f;
        for (int k = 0; k < S; k++) s += __hip_atomic_load(partial + ((size_t)h * S + k) * HD + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[(size_t)h * HD + i] = s;
    }
    if (tid == 0) __hip_atomic_store(arrive + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every other workgroup of this head has arrived: ready for the next launch
}
size_t attn_split_workspace_bytes(int n_head, int hd, int n_ctx, int splits) {
    return (size_t)n_head * (size_t)((n_ctx + 3) & ~3) * 4 + (size_t)n_head * splits * hd * 4 + (size_t)n_head * hd * 2 + (size_t)n_head * 4 + 1024;
}
int attn_split_count(int n_head, int cus) { return std::max(2, std::min(16, (cus - cus / 16) / std::max(1, n_head))); }   // ~240 of 256 CUs: 6 splits for 40 heads, 7 for 32
template <int HD>
static void launch_attn_split_hd(float *q, const float *k, const float *v, __half *kc, __half *vc, int n_head, const int *n_past, int n_ctx, const float *cos_tab, const float *sin_tab,
                                 const Tables &tb, float *out, void *ws, int splits, hipStream_t s) {
    const int ld = (n_ctx + 3) & ~3;
    float *scores = reinterpret_cast<float *>(ws);
    float *partial = scores + (size_t)n_head * ld;
    __half *qrot = reinterpret_cast<__half *>(partial + (size_t)n_head * splits * HD);
    unsigned *arrive = reinterpret_cast<unsigned *>(reinterpret_cast<unsigned char *>(qrot) + (((size_t)n_head * HD * 2 + 255) & ~(size_t)255));
    note_kernel("k_attn_split_scores<%d>", HD);
    hipLaunchKernelGGL((k_attn_split_scores<HD>), dim3((unsigned)n_head, (unsigned)splits), dim3(AS_THREADS), 0, s, q, k, v, kc, vc, n_head * HD, n_past, cos_tab, sin_tab, scores, ld, qrot);
    const size_t lds = (size_t)ld * 4 + (size_t)(AS_THREADS / (HD / 8)) * HD * 4 + 64;
    static bool attr = false;
    if (!attr) { HIP_IGNORE(lds_optin_max(&k_attn_split_pv<HD>)); attr = true; }
    note_kernel("k_attn_split_pv<%d>", HD);
    hipLaunchKernelGGL((k_attn_split_pv<HD>), dim3((unsigned)n_head, (unsigned)splits), dim3(AS_THREADS), lds, s, scores, ld, vc, n_head * HD, n_past, tb, partial, arrive, out);
}
// decode (one row): RoPE + KV append + attention with the keys of every head shared by `splits` workgroups; `ws` >= attn_split_workspace_bytes(...), its last 1 KiB zeroed once
void launch_attn_llm_split(float *q, const float *k, const float *v, __half *kcache, __half *vcache, int n_head, int hd, const int *n_past, int n_ctx, const float *cos_tab,
                           const float *sin_tab, const Tables &tb, float *out, void *ws, int splits, hipStream_t s) {
    attn_for_head_size_or_throw(hd, [&](auto tag) { launch_attn_split_hd<decltype(tag)::value>(q, k, v, kcache, vcache, n_head, n_past, n_ctx, cos_tab, sin_tab, tb, out, ws, splits, s); });
}

// =====================================================================================================================
// Prefill attention (N > 1 query rows of one conversation) on the exact-f32 matrix cores.  The per-token kernel above re-reads a head's whole K and V once per
// query (142 x 40 workgroups per layer for the image-turn prompt: 82 us per layer); here a workgroup owns (head, 16 consecutive queries) and streams the keys the
// LAST of its queries may see through LDS in tiles of 64 -- K once for the scores, V once for the output.
//   scores : v_mfma_f32_16x16x4_f32 over the head dim; operands are the fp16 values (q rounded to fp16, cached k) widened to fp32, so every product is exact and
//            the accumulator is the k-ordered fp32 fma chain of k_attn_llm's dot_row -- bit-identical scores; then * 1/sqrt(hd)
//   softmax: per query over its own causal range: max, fp16-table exp, exact double sum, probabilities rounded to fp16 (as k_attn_llm)
//   output : P V on the same MFMA, keys in index order (k_attn_llm adds key partitions in another order: fp32 rounding only)
// =====================================================================================================================
typedef float pf4_t __attribute__((ext_vector_type(4)));
constexpr int AP_QT = 16, AP_KT = 64;
template <int HD>
__device__ __forceinline__ void ap_stage(float *kv, const __half *__restrict__ cache, int E, int h, int key0, int T, int tid) {
    constexpr int C8 = HD / 8, LDV = HD + 1, PER = AP_KT * C8 / 256;     // 16-byte pieces per thread
    int4 x[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) { const int e = tid + 256 * u, j = e / C8, c = e - j * C8; x[u] = ld16(cache + (size_t)min(key0 + j, T - 1) * E + (size_t)h * HD + 8 * c); }
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int e = tid + 256 * u, j = e / C8, c = e - j * C8;
        const bool live = key0 + j < T;
        const unsigned w[4] = {(unsigned)x[u].x, (unsigned)x[u].y, (unsigned)x[u].z, (unsigned)x[u].w};
        float *d = kv + j * LDV + 8 * c;
#pragma unroll
        for (int i = 0; i < 4; i++) { d[2 * i] = live ? h2f_bits(w[i] & 0xFFFF) : 0.0f; d[2 * i + 1] = live ? h2f_bits(w[i] >> 16) : 0.0f; }
    }
}
// QS = query sub-tiles of 16 per workgroup: 2 from 256 prompt rows on -- the staged key / value tile (the fp16 -> fp32 conversion and its LDS writes are most of the
// kernel's time) then serves 32 queries instead of 16.
template <int HD, int QS>
__global__ __launch_bounds__(256) void k_attn_prefill(const float *__restrict__ q, const __half *__restrict__ kc, const __half *__restrict__ vc, int E, int N, const int *__restrict__ n_past,
                                                      const Tables tb, float *__restrict__ out, int LS) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_ap[];
    constexpr int LDV = HD + 1, KS = HD / 4, DT = HD / 16, QT = AP_QT * QS;
    static_assert(DT % 4 == 0 || DT == 2, "dim tiles are dealt to the 4 waves");
    float *S = reinterpret_cast<float *>(smem_ap);                // [QT][LS]
    float *kv = S + (size_t)QT * LS;                              // [64][LDV]
    const int h = blockIdx.x, q0 = blockIdx.y * QT, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int np = *n_past;
    const int T = np + min(q0 + QT - 1, N - 1) + 1;               // keys the last query of this tile sees
    const int nkt = (T + AP_KT - 1) / AP_KT;
    const float scale = 1.0f / sqrtf((float)HD);
    // Q fragments: A[i = lane & 15 (query)][kk = lane >> 4] per k-step, rounded to fp16 like ggml's f16 x f32 mul_mat
    float qf[QS][KS];
#pragma unroll
    for (int qs = 0; qs < QS; qs++) {
        const float *qp = q + (size_t)min(q0 + 16 * qs + (lane & 15), N - 1) * E + (size_t)h * HD + (lane >> 4);
#pragma unroll
        for (int ks = 0; ks < KS; ks++) qf[qs][ks] = f16r(qp[4 * ks]);
    }
    for (int kt = 0; kt < nkt; kt++) {
        __syncthreads();
        ap_stage<HD>(kv, kc, E, h, kt * AP_KT, T, tid);
        __syncthreads();
        const int key0 = kt * AP_KT + 16 * wave;
        if (key0 < T) {
            const float *kb = kv + (size_t)(16 * wave + (lane & 15)) * LDV + (lane >> 4);
            pf4_t acc[QS];
#pragma unroll
            for (int qs = 0; qs < QS; qs++) acc[qs] = pf4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int ks = 0; ks < KS; ks++) {
                const float kval = kb[4 * ks];
#pragma unroll
                for (int qs = 0; qs < QS; qs++) acc[qs] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[qs][ks], kval, acc[qs], 0, 0, 0);
            }
#pragma unroll
            for (int qs = 0; qs < QS; qs++)
#pragma unroll
                for (int r = 0; r < 4; r++) S[(size_t)(16 * qs + (lane >> 4) * 4 + r) * LS + key0 + (lane & 15)] = acc[qs][r] * scale;
        }
    }
    __syncthreads();
#pragma unroll
    for (int qs = 0; qs < QS; qs++) {   // softmax: 16 lanes per query row; row r sees keys 0 .. np + q0 + r
        const int row = 16 * qs + (tid >> 4), sub = tid & 15;
        const int Tq = min(np + q0 + row + 1, T);
        float *sr = S + (size_t)row * LS;
        float mx = -INFINITY;
        for (int j = sub; j < Tq; j += 16) mx = fmaxf(mx, sr[j]);
        mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2)); mx = fmaxf(mx, __shfl_xor(mx, 4)); mx = fmaxf(mx, __shfl_xor(mx, 8));
        double sum = 0.0;
        for (int j0 = sub; j0 < Tq; j0 += 64) {                  // table gathers in batches of 4
            float e[4];
#pragma unroll
            for (int u = 0; u < 4; u++) e[u] = tab(tb.exp, sr[min(j0 + 16 * u, Tq - 1)] - mx);
#pragma unroll
            for (int u = 0; u < 4; u++) { const int j = j0 + 16 * u; if (j < Tq) { sr[j] = e[u]; sum += (double)e[u]; } }
        }
        sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4); sum += __shfl_xor(sum, 8);
        const float inv = (float)(1.0 / sum);
        for (int j = sub; j < nkt * AP_KT; j += 16) sr[j] = j < Tq ? f16r(sr[j] * inv) : 0.0f;
    }
    // O = P V: wave w owns dim tiles w, w + 4, ..; accumulators persist across the key tiles
    constexpr int DPW = (DT + 3) / 4;
    pf4_t oacc[QS][DPW];
#pragma unroll
    for (int qs = 0; qs < QS; qs++)
#pragma unroll
        for (int i = 0; i < DPW; i++) oacc[qs][i] = pf4_t{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kt = 0; kt < nkt; kt++) {
        __syncthreads();
        ap_stage<HD>(kv, vc, E, h, kt * AP_KT, T, tid);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < DPW; i++) {
            const int dt = wave + 4 * i;
            if (dt < DT) {
                const float *vb = kv + (size_t)(lane >> 4) * LDV + dt * 16 + (lane & 15);
#pragma unroll
                for (int ks = 0; ks < AP_KT / 4; ks++) {
                    const float vval = vb[(size_t)4 * ks * LDV];
#pragma unroll
                    for (int qs = 0; qs < QS; qs++)
                        oacc[qs][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(S[(size_t)(16 * qs + (lane & 15)) * LS + kt * AP_KT + (lane >> 4) + 4 * ks], vval, oacc[qs][i], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int qs = 0; qs < QS; qs++)
#pragma unroll
        for (int i = 0; i < DPW; i++) {
            const int dt = wave + 4 * i;
            if (dt < DT) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int qrow = q0 + 16 * qs + (lane >> 4) * 4 + r;
                    if (qrow < N) out[(size_t)qrow * E + (size_t)h * HD + dt * 16 + (lane & 15)] = oacc[qs][i][r];
                }
            }
        }
}
// =====================================================================================================================
// Prompt attention on the fp16 matrix cores: k_attn_prefill_h<HD, QS> (4 waves, 16 QS queries) and k_attn_prefill_h8<HD> (8 waves, 32 queries).
// The family computes what k_attn_prefill computes, for a workgroup's (head, query tile): every operand of both products IS an fp16 value in the reference (K / V cache
// rows, q rounded to fp16 by ggml's f16 x f32 mul_mat, probabilities rounded to fp16 before P.V), so v_mfma_f32_16x16x32_f16 multiplies them exactly and accumulates in
// fp32.  scores = q K^T / sqrt(hd) into LDS rows S[query][key]; softmax per query over its own causal range (max, fp16-table exp, exact double sum, p = fp16(e / sum));
// out = P V with the key tiles in index order.  fp32 accumulation order inside the MFMA differs from the sequential chain of k_attn_llm / the oracle (fp32 rounding only;
// MINIGPT4_PARITY uses k_attn_ref).
// Every stage is written ONCE, as one of the APH_ macros below; a kernel is only its schedule (loops, barriers, register double buffers, wave roles, MG4_TLP stamps).
// The forms therefore give the same bits: one MFMA chain per (query group, key tile), an order-free max and sum, P.V tiles in key order -- whichever waves run them
// (tests/test_gpu_prefill_batch.py compares them).
// Why text and not __device__ functions: a function is simplified on its own before it is inlined, and the index arithmetic then keeps another form.  With only the
// softmax row behind a forceinline function (the tile as a struct or as scalars; the thread index passed raw or split by the caller) the 4-wave kernels came out up to 22
// instructions away from the ISA that was validated and measured; with every stage behind one, all eighteen instantiations differed.  As macros they are instruction
// for instruction what they were (tools/isa_diff.py) -- what attn_llm_body.hpp found for the decode family.  Even moving APH_TILE below the thread indices renames registers.
// A stage names its threads by its arguments -- st: staging thread 0 .. 255 (tid; the 8-wave form's loader thread lt), mw: MFMA wave 0 .. 3 (wave; mw) -- and is handed
// the LDS buffer it reads or writes.  In scope where one is used: the kernel's parameters, HD, QS, SEG, the names APH_GEOMETRY and APH_TILE_KEYS declare, h, tid, lane, and
// out_h (a parameter of the 8-wave form; the 4-wave form declares a null local, which the compiler drops with the arms that test it).
// =====================================================================================================================
typedef _Float16 aph8_t __attribute__((ext_vector_type(8)));
constexpr int APH_LDT = 70;                                       // halfs per row of a transposed V tile [dim][key]: a lane's 8 consecutive keys of one dim are contiguous
// SEG form (Engine::prefill_batch, trailing AttnSegArgs argument): the rows of several conversations packed in one chunk, one launch.  Grid (head, work item); item y
// = (segment tiles[2 y], first query tiles[2 y + 1]), dealt longest-first over ALL segments by the host (attn_seg_tiles).  Segment i = segs[4 i ..]: slot, first packed
// row, rows, position of its first row.  Each segment is tiled from its own row 0, so a tile sees exactly the queries and keys of the same tile of that segment's own
// launch: the rows are bit-identical.  Only APH_TILE differs; without the argument the kernels are the one-conversation forms.
struct AttnSegArgs { const int *segs; const int *tiles; long long seq_stride; };
#define APH_GEOMETRY                                                                                                                                                    \
    constexpr bool SEG = sizeof...(Seg) > 0;                                                                                                                            \
    constexpr int C8 = HD / 8, QT = AP_QT * QS, KSQ = HD / 32, DT = HD / 16, PER = AP_KT * C8 / 256, DPW = (DT + 3) / 4;                                                \
    static_assert(PER >= 1 && (DT % 4 == 0 || DT == 2), "tile geometry")
// tile set-up.  Causal: the LAST query tile sees the most keys -- it is dispatched first (longest-first), so the short tiles fill the tail of the launch.  SEG: the work
// item (segment, first query) comes from the host's longest-first list instead: the segment's rows, its conversation's cache, its first position
#define APH_TILE                                                                                                                                                        \
    int q0 = (int)(gridDim.y - 1 - blockIdx.y) * QT, np_seg = 0;                                                                                                        \
    if constexpr (SEG) {                                                                                                                                                \
        const AttnSegArgs sa = (seg, ...);                                                                                                                              \
        const int *t = sa.tiles + 2 * blockIdx.y, *g = sa.segs + 4 * t[0];                                                                                              \
        q0 = t[1]; N = g[2]; np_seg = g[3];                                                                                                                             \
        q += (size_t)g[1] * E; out += (size_t)g[1] * E; kc += (size_t)g[0] * sa.seq_stride; vc += (size_t)g[0] * sa.seq_stride;                                         \
        if (out_h) out_h += (size_t)g[1] * E;                                                                                                                           \
    }
// np: first position; T: keys the last query of this tile sees; nkt: key tiles
#define APH_TILE_KEYS                                                                                                                                                   \
    const int np = SEG ? np_seg : *n_past;                                                                                                                              \
    const int T = np + min(q0 + QT - 1, N - 1) + 1;                                                                                                                     \
    const int nkt = (T + AP_KT - 1) / AP_KT;                                                                                                                            \
    const float scale = 1.0f / sqrtf((float)HD);                                                                                                                        \
    const int l15 = lane & 15, l4 = lane >> 4
// Q fragments (A operands) into qf[QS][KSQ]: query l15 of each group of 16, dims 32 ks + 8 l4 .. + 7, rounded to fp16
#define APH_Q_FRAGS                                                                                                                                                     \
    _Pragma("unroll") for (int qs = 0; qs < QS; qs++) {                                                                                                                 \
        const float *qp = q + (size_t)min(q0 + 16 * qs + l15, N - 1) * E + (size_t)h * HD + 8 * l4;                                                                     \
        _Pragma("unroll") for (int ks = 0; ks < KSQ; ks++) {                                                                                                            \
            const float4 a = *reinterpret_cast<const float4 *>(qp + 32 * ks), b = *reinterpret_cast<const float4 *>(qp + 32 * ks + 4);                                  \
            const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};                                                                                                \
            _Pragma("unroll") for (int e = 0; e < 8; e++) qf[qs][ks][e] = (_Float16)__half2float(f2h_rn(v[e]));                                                         \
        }                                                                                                                                                               \
    }
// key tile `tile` of the cache `base` (kc or vc), global -> registers X[PER] (rows past the last key repeat it)
#define APH_KV_LOAD(X, base, tile, st)                                                                                                                                  \
    _Pragma("unroll") for (int u = 0; u < PER; u++) { const int e = (st) + 256 * u, j = e / C8, c = e - j * C8;                                                         \
        X[u] = ld16(base + (size_t)min((tile) * AP_KT + j, T - 1) * E + (size_t)h * HD + 8 * c); }
// K tile, registers X -> Kt [64][HD] as it is: 16-byte chunk c of key j at slot c ^ (j & (C8 - 1)) (conflict-free fragment reads in APH_SCORES)
#define APH_K_WRITE(Kt, X, st)                                                                                                                                          \
    _Pragma("unroll") for (int u = 0; u < PER; u++) { const int e = (st) + 256 * u, j = e / C8, c = e - j * C8;                                                         \
        *reinterpret_cast<int4 *>(Kt + j * HD + ((c ^ (j & (C8 - 1))) << 3)) = X[u]; }
// scores of (MFMA wave mw, key tile kt) out of Kt: keys kt 64 + 16 mw .. + 15 against the QS query groups, one MFMA chain over the head dim each, * scale, into S
#define APH_SCORES(Kt, kt, mw)                                                                                                                                          \
    const int key0 = (kt) * AP_KT + 16 * (mw);                                                                                                                          \
    if (key0 < T) {                                                                                                                                                     \
        const int row = 16 * (mw) + l15;                                                                                                                                \
        pf4_t acc[QS];                                                                                                                                                  \
        _Pragma("unroll") for (int qs = 0; qs < QS; qs++) acc[qs] = pf4_t{0.0f, 0.0f, 0.0f, 0.0f};                                                                      \
        _Pragma("unroll") for (int ks = 0; ks < KSQ; ks++) {                                                                                                            \
            const aph8_t kf = *reinterpret_cast<const aph8_t *>(Kt + row * HD + (((4 * ks + l4) ^ (row & (C8 - 1))) << 3));                                             \
            _Pragma("unroll") for (int qs = 0; qs < QS; qs++) acc[qs] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[qs][ks], kf, acc[qs], 0, 0, 0);                       \
        }                                                                                                                                                               \
        _Pragma("unroll") for (int qs = 0; qs < QS; qs++)                                                                                                               \
            _Pragma("unroll") for (int r = 0; r < 4; r++) S[(size_t)(16 * qs + l4 * 4 + r) * LS + key0 + l15] = acc[qs][r] * scale;                                     \
    }
// softmax of the tile's query row ROW by 16 lanes; lane `sub` owns the keys 64 s + 4 sub .. + 3 (16-byte LDS accesses); the row sees keys 0 .. np + q0 + ROW.  Same
// values as k_attn_prefill's loop (max, fp16-table exp, exact double sum -- order-free --, p = fp16(e * (1 / sum))) with 16 table gathers in flight per round.
// "a block past the end repeats the last one": its values are dropped by the `j0 + 64 * u < nb` test, which is uniform over the 16 lanes of a row.
// (The table stays in global memory: an LDS copy -- 39 KB by LDS-DMA per workgroup -- left this phase at 8.0 us against 7.7 and cost the 142-row launch its co-resident
//  workgroups, 11.3 -> 15.1 us: the phase is bound by its ~30 vector instructions per element, not by the gathers.)
#define APH_SOFTMAX_ROW(ROW)                                                                                                                                            \
    const int row = (ROW), sub = tid & 15;                                                                                                                              \
    const int Tq = min(np + q0 + row + 1, T), nb = nkt * AP_KT;                                                                                                         \
    float *sr = S + (size_t)row * LS;                                                                                                                                   \
    float mx = -INFINITY;                                                                                                                                               \
    for (int j = 4 * sub; j < nb; j += 64) {                                                                                                                            \
        const float4 v = *reinterpret_cast<const float4 *>(sr + j);                                                                                                     \
        mx = fmaxf(mx, j < Tq ? v.x : -INFINITY); mx = fmaxf(mx, j + 1 < Tq ? v.y : -INFINITY); mx = fmaxf(mx, j + 2 < Tq ? v.z : -INFINITY); mx = fmaxf(mx, j + 3 < Tq ? v.w : -INFINITY); \
    }                                                                                                                                                                   \
    mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2)); mx = fmaxf(mx, __shfl_xor(mx, 4)); mx = fmaxf(mx, __shfl_xor(mx, 8));                         \
    double sum = 0.0;                                                                                                                                                   \
    for (int j0 = 0; j0 < nb; j0 += 256) {                                                                                                                              \
        float x[16]; unsigned short t[16];                                                                                                                              \
        _Pragma("unroll") for (int u = 0; u < 4; u++) {                                                                                                                 \
            const int jj = min(j0 + 64 * u, nb - 64) + 4 * sub;          /* a block past the end repeats the last one */                                                \
            const float4 v = *reinterpret_cast<const float4 *>(sr + jj);                                                                                                \
            x[4 * u] = v.x; x[4 * u + 1] = v.y; x[4 * u + 2] = v.z; x[4 * u + 3] = v.w;                                                                                 \
        }                                                                                                                                                               \
        _Pragma("unroll") for (int e = 0; e < 16; e++) {                                                                                                                \
            const int jj = j0 + 64 * (e >> 2) + 4 * sub + (e & 3);                                                                                                      \
            t[e] = reinterpret_cast<const unsigned short *>(tb.exp)[f2h_bits(jj < Tq ? x[e] - mx : 0.0f)];                                                              \
        }                                                                                                                                                               \
        _Pragma("unroll") for (int u = 0; u < 4; u++) {                                                                                                                 \
            const int jj = j0 + 64 * u + 4 * sub;                                                                                                                       \
            if (j0 + 64 * u < nb) {                                                                                                                                     \
                float4 ev;                                                                                                                                              \
                ev.x = jj < Tq ? h2f_bits(t[4 * u]) : 0.0f; ev.y = jj + 1 < Tq ? h2f_bits(t[4 * u + 1]) : 0.0f; ev.z = jj + 2 < Tq ? h2f_bits(t[4 * u + 2]) : 0.0f; ev.w = jj + 3 < Tq ? h2f_bits(t[4 * u + 3]) : 0.0f; \
                sum += (double)ev.x; sum += (double)ev.y; sum += (double)ev.z; sum += (double)ev.w;                                                                     \
                *reinterpret_cast<float4 *>(sr + jj) = ev;                                                                                                              \
            }                                                                                                                                                           \
        }                                                                                                                                                               \
    }                                                                                                                                                                   \
    sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4); sum += __shfl_xor(sum, 8);                                                         \
    const float inv = (float)(1.0 / sum);                                                                                                                               \
    for (int j = 4 * sub; j < nb; j += 64) {                             /* keys past the row's limit already hold 0 */                                                 \
        float4 v = *reinterpret_cast<float4 *>(sr + j);                                                                                                                 \
        v.x = f16r(v.x * inv); v.y = f16r(v.y * inv); v.z = f16r(v.z * inv); v.w = f16r(v.w * inv);                                                                     \
        *reinterpret_cast<float4 *>(sr + j) = v;                                                                                                                        \
    }
// V tile kt, registers X -> Vt TRANSPOSED [HD][APH_LDT]; keys past the last one are written as 0
#define APH_V_WRITE(Vt, X, kt, st)                                                                                                                                      \
    _Pragma("unroll") for (int u = 0; u < PER; u++) {                                                                                                                   \
        const int e = (st) + 256 * u, j = e / C8, c = e - j * C8;                                                                                                       \
        const bool live = (kt) * AP_KT + j < T;                                                                                                                         \
        const unsigned w[4] = {(unsigned)X[u].x, (unsigned)X[u].y, (unsigned)X[u].z, (unsigned)X[u].w};                                                                 \
        unsigned short *d = reinterpret_cast<unsigned short *>(Vt) + (8 * c) * APH_LDT + j;                                                                             \
        _Pragma("unroll") for (int i = 0; i < 4; i++) { d[(2 * i) * APH_LDT] = live ? (unsigned short)(w[i] & 0xFFFF) : (unsigned short)0; d[(2 * i + 1) * APH_LDT] = live ? (unsigned short)(w[i] >> 16) : (unsigned short)0; } \
    }
// P.V of key tile kt out of Vt: MFMA wave mw owns the dim tiles mw, mw + 4, ..; the accumulators oacc[QS][DPW] persist across the key tiles.  (Vt rows are 140 bytes:
// 4-byte aligned loads)
#define APH_PV(Vt, kt, mw)                                                                                                                                              \
    _Pragma("unroll") for (int i = 0; i < DPW; i++) {                                                                                                                   \
        const int dt = (mw) + 4 * i;                                                                                                                                    \
        if (dt < DT) {                                                                                                                                                  \
            _Pragma("unroll") for (int k2 = 0; k2 < AP_KT / 32; k2++) {                                                                                                 \
                const unsigned *vp = reinterpret_cast<const unsigned *>(Vt + (16 * dt + l15) * APH_LDT + 32 * k2 + 8 * l4);                                             \
                union { unsigned u[4]; aph8_t v; } vb;                                                                                                                  \
                _Pragma("unroll") for (int e = 0; e < 4; e++) vb.u[e] = vp[e];                                                                                          \
                _Pragma("unroll") for (int qs = 0; qs < QS; qs++) {                                                                                                     \
                    const float *pp = S + (size_t)(16 * qs + l15) * LS + (kt) * AP_KT + 32 * k2 + 8 * l4;                                                               \
                    const float4 a = *reinterpret_cast<const float4 *>(pp), b = *reinterpret_cast<const float4 *>(pp + 4);                                              \
                    aph8_t pf;                                                                                                                                          \
                    pf[0] = (_Float16)a.x; pf[1] = (_Float16)a.y; pf[2] = (_Float16)a.z; pf[3] = (_Float16)a.w; pf[4] = (_Float16)b.x; pf[5] = (_Float16)b.y; pf[6] = (_Float16)b.z; pf[7] = (_Float16)b.w; \
                    oacc[qs][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf, vb.v, oacc[qs][i], 0, 0, 0);                                                               \
                }                                                                                                                                                       \
            }                                                                                                                                                           \
        }                                                                                                                                                               \
    }
#define APH_ZERO_OACC                                                                                                                                                   \
    pf4_t oacc[QS][DPW];                                                                                                                                                \
    _Pragma("unroll") for (int qs = 0; qs < QS; qs++)                                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < DPW; i++) oacc[qs][i] = pf4_t{0.0f, 0.0f, 0.0f, 0.0f}
// store of MFMA wave mw.  out_h given (8-wave form): the rows as the consumer wants them (an F16 wo multiplies the fp16-rounded attention output: the conversion launch
// is saved), pairs of dims from neighbouring lanes as 4-byte stores; else the f32 rows
#define APH_STORE(mw)                                                                                                                                                   \
    _Pragma("unroll") for (int qs = 0; qs < QS; qs++)                                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < DPW; i++) {                                                                                                               \
            const int dt = (mw) + 4 * i;                                                                                                                                \
            if (dt < DT) {                                                                                                                                              \
                _Pragma("unroll") for (int r = 0; r < 4; r++) {                                                                                                         \
                    const int qrow = q0 + 16 * qs + l4 * 4 + r;                                                                                                         \
                    if (out_h) {                                                                                                                                        \
                        const float o0 = oacc[qs][i][r], o1 = __shfl_xor(o0, 1);                                                                                        \
                        if (qrow < N && !(l15 & 1)) *reinterpret_cast<__half2 *>(out_h + (size_t)qrow * E + (size_t)h * HD + dt * 16 + l15) = __halves2half2(f2h_rn(o0), f2h_rn(o1)); \
                    } else if (qrow < N) out[(size_t)qrow * E + (size_t)h * HD + dt * 16 + l15] = oacc[qs][i][r];                                                       \
                }                                                                                                                                                       \
            }                                                                                                                                                           \
        }
// ---- the 4-wave schedule: every wave stages and multiplies.  Per key tile [barrier, LDS write of the staged tile, global loads of tile kt + 1 (register double buffer:
// one exposed memory round trip per phase instead of one per tile), barrier, MFMAs]; the softmax takes 16 rows at a time.
template <int HD, int QS, typename... Seg>
__global__ __launch_bounds__(256) void k_attn_prefill_h(const float *__restrict__ q, const __half *__restrict__ kc, const __half *__restrict__ vc, int E, int N, const int *__restrict__ n_past,
                                                        const Tables tb, float *__restrict__ out, int LS, const Seg... seg) {
    APH_GEOMETRY;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_aph[];
    float *S = reinterpret_cast<float *>(smem_aph);               // [QT][LS], LS = 4 mod 64
    __half *Kt = reinterpret_cast<__half *>(S + (size_t)QT * LS); // [64][HD]
    __half *Vt = Kt + AP_KT * HD;                                 // [HD][APH_LDT]
    __half *out_h = nullptr;                                      // no fp16 store arm: the compiler drops it
    APH_TILE
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    MG4_TLP(0);
    APH_TILE_KEYS;
    aph8_t qf[QS][KSQ];
    APH_Q_FRAGS
    int4 xk[PER];
    APH_KV_LOAD(xk, kc, 0, tid)
    for (int kt = 0; kt < nkt; kt++) {
        __syncthreads();
        APH_K_WRITE(Kt, xk, tid)
        APH_KV_LOAD(xk, kc, kt + 1, tid)
        __syncthreads();
        APH_SCORES(Kt, kt, wave)
    }
    __syncthreads();
    MG4_TLP(1);
#pragma unroll
    for (int qs = 0; qs < QS; qs++) { APH_SOFTMAX_ROW(16 * qs + (tid >> 4)) }
    MG4_TLP(2);
    APH_ZERO_OACC;
    int4 xv[PER];
    APH_KV_LOAD(xv, vc, 0, tid)
    for (int kt = 0; kt < nkt; kt++) {
        __syncthreads();
        APH_V_WRITE(Vt, xv, kt, tid)
        APH_KV_LOAD(xv, vc, kt + 1, tid)
        __syncthreads();
        APH_PV(Vt, kt, wave)
    }
    MG4_TLP(3);
    APH_STORE(wave)
#ifdef MG4_TIMELINE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    MG4_TLP(4);
#endif
}
// ---- the 8-wave schedule (32 queries): a 512-thread workgroup whose waves have ROLES.  The timeline of the 4-wave form had a 512-key workgroup at 6.2 us of scores +
// 7.7 us of softmax + 12.7 us of P.V, each key tile paying its barriers, LDS write and MFMAs in sequence on the same four waves.  Here waves 4..7 are LOADERS (global ->
// registers two tiles ahead -> LDS tile kt) while waves 0..3 multiply tile kt - 1 out of the OTHER LDS buffer: one barrier per tile and the staging runs beside the MFMAs;
// the softmax uses all 512 threads (32 rows x 16 lanes at once), and the first two V tiles are requested before it.  It also has the fp16 store arm (out_h).
// MINIGPT4_ATTN_PREFILL_W8=0 selects the 4-wave form (A/B).
template <int HD, typename... Seg>
__global__ __launch_bounds__(512) void k_attn_prefill_h8(const float *__restrict__ q, const __half *__restrict__ kc, const __half *__restrict__ vc, int E, int N, const int *__restrict__ n_past,
                                                         const Tables tb, float *__restrict__ out, int LS, __half *__restrict__ out_h, const Seg... seg) {
    constexpr int QS = 2;
    APH_GEOMETRY;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_aph8[];
    constexpr int KVB = (AP_KT * HD * 2 > HD * APH_LDT * 2 ? AP_KT * HD * 2 : HD * APH_LDT * 2);        // bytes of one K (or transposed V) tile buffer
    float *S = reinterpret_cast<float *>(smem_aph8);                                                 // [QT][LS]
    unsigned char *kvb = smem_aph8 + (size_t)QT * LS * 4;                                             // two tile buffers (K tiles, later V tiles)
    APH_TILE
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = wave >= 4;
    const int lt = tid & 255, mw = wave & 3;                                                           // loader thread / MFMA wave index
    MG4_TLP(0);
    APH_TILE_KEYS;
    aph8_t qf[QS][KSQ];
    if (!loader) { APH_Q_FRAGS }
    // ---- scores: iteration kt stages tile kt (loaders) and multiplies tile kt - 1 (MFMA waves)
    int4 xa[PER], xb[PER];                                                                            // loaders: tiles kt and kt + 1 in flight
    if (loader) { APH_KV_LOAD(xa, kc, 0, lt) APH_KV_LOAD(xb, kc, 1, lt) }
    auto k_write = [&](const int4 (&X)[PER], int buf) { __half *Kt = reinterpret_cast<__half *>(kvb + (size_t)buf * KVB); APH_K_WRITE(Kt, X, lt) };
    auto k_mul = [&](int kt, int buf) { const __half *Kt = reinterpret_cast<const __half *>(kvb + (size_t)buf * KVB); APH_SCORES(Kt, kt, mw) };
    for (int kt = 0; kt <= nkt; kt += 2) {
        if (loader) { if (kt < nkt) { k_write(xa, 0); APH_KV_LOAD(xa, kc, kt + 2, lt) } }
        else if (kt >= 1) k_mul(kt - 1, 1);
        __syncthreads();
        if (kt + 1 > nkt) break;
        if (loader) { if (kt + 1 < nkt) { k_write(xb, 1); APH_KV_LOAD(xb, kc, kt + 3, lt) } }
        else k_mul(kt, 0);
        __syncthreads();
    }
    MG4_TLP(1);
    if (loader) { APH_KV_LOAD(xa, vc, 0, lt) APH_KV_LOAD(xb, vc, 1, lt) }                             // the first two V tiles arrive while the softmax runs
    { APH_SOFTMAX_ROW(tid >> 4) }
    MG4_TLP(2);
    // ---- P.V: the same two-role loop over the V tiles
    APH_ZERO_OACC;
    auto v_write = [&](const int4 (&X)[PER], int kt, int buf) { __half *Vt = reinterpret_cast<__half *>(kvb + (size_t)buf * KVB); APH_V_WRITE(Vt, X, kt, lt) };
    auto v_mul = [&](int kt, int buf) { const __half *Vt = reinterpret_cast<const __half *>(kvb + (size_t)buf * KVB); APH_PV(Vt, kt, mw) };
    __syncthreads();                                                     // normalised probabilities visible; the K buffers are free
    for (int kt = 0; kt <= nkt; kt += 2) {
        if (loader) { if (kt < nkt) { v_write(xa, kt, 0); APH_KV_LOAD(xa, vc, kt + 2, lt) } }
        else if (kt >= 1) v_mul(kt - 1, 1);
        __syncthreads();
        if (kt + 1 > nkt) break;
        if (loader) { if (kt + 1 < nkt) { v_write(xb, kt + 1, 1); APH_KV_LOAD(xb, vc, kt + 3, lt) } }
        else v_mul(kt, 0);
        __syncthreads();
    }
    MG4_TLP(3);
    if (!loader) { APH_STORE(mw) }
#ifdef MG4_TIMELINE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    MG4_TLP(4);
#endif
}
#undef APH_GEOMETRY
#undef APH_TILE
#undef APH_TILE_KEYS
#undef APH_Q_FRAGS
#undef APH_KV_LOAD
#undef APH_K_WRITE
#undef APH_SCORES
#undef APH_SOFTMAX_ROW
#undef APH_V_WRITE
#undef APH_PV
#undef APH_ZERO_OACC
#undef APH_STORE
// ---- launchers.  Forms: 1 = k_attn_prefill_h8, 2 = k_attn_prefill_h<HD, 2>, 3 = k_attn_prefill_h<HD, 1>, 4 = the exact-f32 k_attn_prefill<HD, 1>
// (LaunchTuning::attn_prefill_w8 / _f16 / _form choose among them)
// the LDS image of a form for score rows of t_max keys: *LS = floats per score row; returns its bytes, 0 when it exceeds the 160 KiB of a CU (the form refuses).
// Forms 1 .. 3: score rows + fp16 K tile + transposed V tile (form 1: two buffers that hold either); form 4: score rows + one f32 tile.
static size_t attn_prefill_lds(int form, int hd, int t_max, int *LS) {
    *LS = ((t_max + AP_KT - 1) / AP_KT) * AP_KT + (form == 4 ? 1 : 4);
    const size_t rows = (size_t)AP_QT * (form <= 2 ? 2 : 1) * *LS * 4, kt = (size_t)AP_KT * hd * 2, vt = (size_t)hd * APH_LDT * 2;
    const size_t lds = rows + (form == 1 ? 2 * std::max(kt, vt) : form == 4 ? (size_t)AP_KT * (hd + 1) * 4 : kt + vt);
    return lds > 160 * 1024 - 512 ? 0 : lds;
}
// the fp16 forms in the order they are tried.  wide: 32 queries per staged K / V tile still give every CU a workgroup
static int attn_prefill_forms(const LaunchTuning &tune, bool wide, int (&forms)[3]) {
    const int f = tune.attn_prefill_form;
    int n = 0;
    if (f == 1 || (f == 0 && tune.attn_prefill_w8 && wide)) forms[n++] = 1;
    if (f == 2 || (f == 0 && wide)) forms[n++] = 2;
    if (f == 0 || f == 3) forms[n++] = 3;
    return n;
}
// one fp16 form over `tiles` query tiles: of one conversation (N rows at *n_past), or with a trailing AttnSegArgs of the segments of a packed chunk (N = 0, no n_past).
// false: its LDS image does not fit
template <int HD, int FORM, typename... Seg>
static bool launch_attn_prefill_form(const float *q, const __half *kc, const __half *vc, int N, int n_head, const int *n_past, int t_max, int tiles, const Tables &tb, float *out, hipStream_t s,
                                     __half *out_h, const Seg... seg) {
    int LS;
    const size_t lds = attn_prefill_lds(FORM, HD, t_max, &LS);
    if (!lds) return false;
    const dim3 grid((unsigned)n_head, (unsigned)tiles);
    static bool attr = false;
    if constexpr (FORM == 1) {
        if (!attr) { HIP_IGNORE(lds_optin_max(&k_attn_prefill_h8<HD, Seg...>)); attr = true; }
        if constexpr (sizeof...(Seg) > 0) note_kernel("k_attn_prefill_h8<%d, SEG>", HD);
        hipLaunchKernelGGL((k_attn_prefill_h8<HD, Seg...>), grid, dim3(512), lds, s, q, kc, vc, n_head * HD, N, n_past, tb, out, LS, out_h, seg...);
    } else {
        constexpr int QS = FORM == 2 ? 2 : 1;
        if (!attr) { HIP_IGNORE(lds_optin_max(&k_attn_prefill_h<HD, QS, Seg...>)); attr = true; }
        if constexpr (sizeof...(Seg) > 0) note_kernel("k_attn_prefill_h<%d, %d, SEG>", HD, QS);
        hipLaunchKernelGGL((k_attn_prefill_h<HD, QS, Seg...>), grid, dim3(256), lds, s, q, kc, vc, n_head * HD, N, n_past, tb, out, LS, seg...);
    }
    return true;
}
// the first fp16 form of attn_prefill_forms that fits; sg: the segments of a packed chunk, nullptr: one conversation.  *wrote_h: the 8-wave form ran and stored fp16 rows
template <int HD>
static bool launch_attn_prefill_f16(const float *q, const __half *kc, const __half *vc, int N, int n_head, const int *n_past, int t_max, const AttnSegs *sg, const Tables &tb, float *out,
                                    const LaunchTuning &tune, hipStream_t s, __half *out_h, bool *wrote_h) {
    auto tiles = [&](int qs) { return sg ? sg->n_tiles[qs - 1] : (N + AP_QT * qs - 1) / (AP_QT * qs); };
    auto launch = [&](auto form) {
        constexpr int FORM = decltype(form)::value, QS = FORM == 3 ? 1 : 2;
        __half *oh = FORM == 1 ? out_h : nullptr;                      // only the 8-wave form has the fp16 store arm
        if (sg) return launch_attn_prefill_form<HD, FORM>(q, kc, vc, 0, n_head, nullptr, t_max, tiles(QS), tb, out, s, oh, AttnSegArgs{sg->segs, sg->tiles[QS - 1], (long long)sg->seq_stride});
        return launch_attn_prefill_form<HD, FORM>(q, kc, vc, N, n_head, n_past, t_max, tiles(QS), tb, out, s, oh);
    };
    int forms[3];
    const int n = attn_prefill_forms(tune, n_head * tiles(2) >= 256, forms);
    for (int i = 0; i < n; i++) {
        const int f = forms[i];
        if (f == 1 ? launch(std::integral_constant<int, 1>{}) : f == 2 ? launch(std::integral_constant<int, 2>{}) : launch(std::integral_constant<int, 3>{})) {
            if (f == 1 && wrote_h) *wrote_h = out_h != nullptr;
            return true;
        }
    }
    return false;
}
// Fallback: k_attn_prefill<HD, 1>, the round-2 kernel with fp32 score / value products.  Taken (a) with LaunchTuning::attn_prefill_f16 == 0 (test library: the A/B switch of
// the fp16 kernels), (b) when the fp16 kernels refuse because their LDS image exceeds the 160 KiB of a CU.  Both forms hold 16 score rows of the whole context: at head
// size 128 both end at 1984 keys; beyond, this returns false and Engine::forward runs the rows through the decode attention kernel (k_attn_llm, one query row per
// workgroup), which has no such limit.
// (QS = 2 -- 32 queries per staged key / value tile from 256 prompt rows on -- is bit-identical and was measured 2 % SLOWER at 512 rows: 13B Q5_K_M 31.7 vs 31.0 ms,
// 13B f16 27.9 vs 27.2 ms, profiles/r02r_prefill_ksplit_fill_sweep.log; half the workgroups, each twice as long: not instantiated.)
template <int HD>
static bool launch_attn_prefill_f32(const float *q, const __half *kc, const __half *vc, int N, int n_head, const int *n_past, int t_max, const Tables &tb, float *out, hipStream_t s) {
    int LS;
    const size_t lds = attn_prefill_lds(4, HD, t_max, &LS);
    if (!lds) return false;
    static bool attr = false;
    if (!attr) { HIP_IGNORE(lds_optin_max(&k_attn_prefill<HD, 1>)); attr = true; }
    hipLaunchKernelGGL((k_attn_prefill<HD, 1>), dim3((unsigned)n_head, (unsigned)((N + AP_QT - 1) / AP_QT)), dim3(256), lds, s, q, kc, vc, n_head * HD, N, n_past, tb, out, LS);
    return true;
}
// Segmented prompt attention (Engine::prefill_batch): one launch over every segment of a packed chunk; the same forms and the same size rule as launch_attn_prefill,
// with the 32-query work items of all segments standing in for one conversation's tiles.
int attn_seg_tiles(const int *segs, int n_seg, int qt, int *out) {
    struct Item { int seg, q0, keys; };
    std::vector<Item> v;
    for (int i = 0; i < n_seg; i++)
        for (int q0 = 0; q0 < segs[4 * i + 2]; q0 += qt) v.push_back({i, q0, segs[4 * i + 3] + std::min(q0 + qt, segs[4 * i + 2])});
    // longest first over all segments (a lone segment: its last tile first, as the one-conversation launch deals them); ties keep the segment order
    std::stable_sort(v.begin(), v.end(), [](const Item &a, const Item &b) { return a.keys > b.keys; });
    for (size_t k = 0; k < v.size(); k++) { out[2 * k] = v[k].seg; out[2 * k + 1] = v[k].q0; }
    return (int)v.size();
}
bool launch_attn_prefill_seg(const float *q, const __half *kcache, const __half *vcache, const AttnSegs &sg, int n_head, int hd, const Tables &tb, float *out, const LaunchTuning &tune, hipStream_t s,
                             __half *out_h, bool *wrote_h) {
    if (wrote_h) *wrote_h = false;
    bool done = false;                                             // an unsupported head size: declined, like a shape that does not fit
    if (!tune.attn_prefill_f16) return false;                        // the exact-f32 kernel: per-segment launches (the caller)
    attn_for_head_size(hd, [&](auto tag) { done = launch_attn_prefill_f16<decltype(tag)::value>(q, kcache, vcache, 0, n_head, nullptr, sg.t_max, &sg, tb, out, tune, s, out_h, wrote_h); });
    return done;
}
// N > 1 query rows at positions *n_past .. *n_past + N - 1 (launch_rope_kv has run); t_max >= *n_past + N (the host's view, sizes the LDS score rows).
// false -> the score rows do not fit LDS (very long contexts): the caller runs launch_attn_llm instead.
bool launch_attn_prefill(const float *q, const __half *kcache, const __half *vcache, int N, int n_head, int hd, const int *n_past, int t_max, const Tables &tb, float *out, const LaunchTuning &tune,
                         hipStream_t s, __half *out_h, bool *wrote_h) {
    if (wrote_h) *wrote_h = false;
    bool done = false;
    attn_for_head_size(hd, [&](auto tag) {
        constexpr int HD = decltype(tag)::value;
        done = (tune.attn_prefill_f16 && launch_attn_prefill_f16<HD>(q, kcache, vcache, N, n_head, n_past, t_max, nullptr, tb, out, tune, s, out_h, wrote_h)) ||
               launch_attn_prefill_f32<HD>(q, kcache, vcache, N, n_head, n_past, t_max, tb, out, s);
    });
    return done;
}
bool attn_head_size_supported(int hd) { return hd == 32 || hd == 64 || hd == 128; }

// =====================================================================================================================
// MINIGPT4_PARITY=1 attention: the oracle's loops (oracle/refcpu.c orc_llama_eval, = ggml's mul_mat(K, Q) / soft_max / mul_mat(V, P) on f16 operands) with every fp32
// chain in ITS order: thread = one key for the scores (sequential fma over the head dimension), exact double sum for the softmax, thread = one output
// dimension for P.V (sequential fma over the keys).  After launch_rope_kv (q rotated in place, caches appended).  One workgroup per (head, query row).
// =====================================================================================================================
// FUSED (one query row, decode): q | k | v are the raw projections; RoPE and the cache append (k_rope_kv's arithmetic) happen here, the new key / value row is also kept in LDS
// (the cache line written by this workgroup is not read back).  P.V: the value rows travel through LDS in chunks of 128 keys (16-byte coalesced loads, the next chunk in
// registers while this one is chained) -- a thread's chain over the keys is unchanged, it no longer waits for a strided 2-byte load per key.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_attn_ref(const float *__restrict__ q, const float *__restrict__ kraw, const float *__restrict__ vraw, __half *__restrict__ kc, __half *__restrict__ vc,
                                                  int E, int hd, const int *__restrict__ n_past, const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, const Tables tb, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_ref[];
    const int h = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int T = *n_past + t + 1;
    constexpr int CH = 128;                                       // keys per value chunk
    __half *vbuf = reinterpret_cast<__half *>(smem_ref);          // [2][CH][hd]
    float *sc = reinterpret_cast<float *>(vbuf + 2 * CH * hd);    // [T]
    __half *ph = reinterpret_cast<__half *>(sc + ((T + 3) & ~3)); // [T]
    __half *qh = ph + ((T + 7) & ~7);                             // [hd]
    __half *knew = qh + hd, *vnew = knew + hd;                    // [hd] each (FUSED)
    __shared__ float red_f[4]; __shared__ double red_d[4];
    if (FUSED) {
        if (tid < hd / 2) {
            const int i = tid, pos = T - 1;
            const float c = cos_tab[(size_t)pos * (hd / 2) + i], s = sin_tab[(size_t)pos * (hd / 2) + i];
            const size_t o = (size_t)h * hd + 2 * i;
            const float2 qr = rope_rot(q[o], q[o + 1], c, s);
            qh[2 * i] = f2h_rn(qr.x); qh[2 * i + 1] = f2h_rn(qr.y);
            const size_t co = (size_t)pos * E + (size_t)h * hd + 2 * i;
            const __half2 kk = rope_rot_h2(kraw[o], kraw[o + 1], c, s), vv = __floats2half2_rn(vraw[o], vraw[o + 1]);
            st_h2(kc + co, kk); st_h2(vc + co, vv);
            st_h2(knew + 2 * i, kk); st_h2(vnew + 2 * i, vv);
        }
    } else {
        for (int i = tid; i < hd; i += 256) qh[i] = __float2half_rn(q[(size_t)t * E + (size_t)h * hd + i]);
    }
    __syncthreads();
    const float kq_scale = 1.0f / sqrtf((float)hd);
    float mx = -INFINITY;
    for (int j = tid; j < T; j += 256) {                          // the row in 16-byte pieces (hd % 8 == 0), the fma chain in element order as before
        const __half *kr = (FUSED && j == T - 1) ? knew : kc + (size_t)j * E + (size_t)h * hd;
        float s = 0.0f;
        for (int i0 = 0; i0 < hd; i0 += 32) {
            int4 kk[4];
#pragma unroll
            for (int c = 0; c < 4; c++) kk[c] = i0 + 8 * c < hd ? ld16(kr + i0 + 8 * c) : make_int4(0, 0, 0, 0);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (i0 + 8 * c >= hd) break;
                const unsigned wds[4] = {(unsigned)kk[c].x, (unsigned)kk[c].y, (unsigned)kk[c].z, (unsigned)kk[c].w};
#pragma unroll
                for (int e = 0; e < 4; e++) { const int i = i0 + 8 * c + 2 * e; s = fmaf(h2f_bits(wds[e] & 0xFFFF), __half2float(qh[i]), s); s = fmaf(h2f_bits(wds[e] >> 16), __half2float(qh[i + 1]), s); }
            }
        }
        s *= kq_scale; sc[j] = s; mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red_f[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
    double sum = 0.0;
    for (int j = tid; j < T; j += 256) { const float v = tab(tb.exp, sc[j] - mx); sc[j] = v; sum += (double)v; }   // <= 2048 fp16 values: the double sum is exact in any order
    sum = wave_sum_d(sum);
    if ((tid & 63) == 0) red_d[tid >> 6] = sum;
    __syncthreads();
    const float inv = (float)(1.0 / (((red_d[0] + red_d[1]) + red_d[2]) + red_d[3]));
    for (int j = tid; j < T; j += 256) ph[j] = f2h_rn(sc[j] * inv);
    // ---- P.V: chunk c = keys c CH .. of this head's value rows -> LDS; 16 threads x 16 bytes cover a row's hd (= 128) halves, 16 keys per pass of the workgroup
    const int per_row = hd / 8, keys_per_pass = 256 / per_row, passes = CH / keys_per_pass;   // hd = 128: 16, 16, 8; hd = 64: 8, 32, 4; hd = 32: 4, 64, 2
    const int kr_ = tid / per_row, part = tid - kr_ * per_row;
    const int n_chunks = (T + CH - 1) / CH;
    int4 stage[8];
    auto request = [&](int c) {
#pragma unroll
        for (int p = 0; p < 8; p++) if (p < passes) {
            const int j = min(c * CH + p * keys_per_pass + kr_, T - 1);                     // clamped: rows past T are never chained
            const __half *src = (FUSED && j == T - 1) ? vnew + part * 8 : vc + (size_t)j * E + (size_t)h * hd + part * 8;
            stage[p] = ld16(src);
        }
    };
    auto deposit = [&](int b) {
#pragma unroll
        for (int p = 0; p < 8; p++) if (p < passes) *reinterpret_cast<int4 *>(vbuf + ((size_t)b * CH + p * keys_per_pass + kr_) * hd + part * 8) = stage[p];
    };
    request(0);
    __syncthreads();                                              // ph complete (and knew / vnew visible)
    deposit(0);
    float s = 0.0f;
    for (int c = 0; c < n_chunks; c++) {
        __syncthreads();                                          // chunk c deposited; everybody has left the buffer chunk c + 1 goes to
        if (c + 1 < n_chunks) request(c + 1);
        if (tid < hd) {
            const __half *vb = vbuf + (size_t)(c & 1) * CH * hd + tid;
            const int j0 = c * CH, n = min(CH, T - j0);
            for (int u = 0; u < n; u++) s = fmaf(__half2float(vb[(size_t)u * hd]), __half2float(ph[j0 + u]), s);   // key order
        }
        if (c + 1 < n_chunks) deposit((c + 1) & 1);
    }
    if (tid < hd) out[(size_t)t * E + (size_t)h * hd + tid] = s;
}
static size_t attn_ref_lds(int t_max, int hd) { return (size_t)2 * 128 * hd * 2 + (size_t)((t_max + 3) & ~3) * 4 + (size_t)((t_max + 7) & ~7) * 2 + (size_t)hd * 2 * 3 + 64; }
// largest n_ctx whose score / probability rows fit k_attn_ref's LDS next to its value staging (parity mode): smaller than attn_max_ctx(hd), which is the fast kernel's
constexpr size_t ATTN_REF_DYN_LDS = 160 * 1024 - 512;                     // the CU's 160 KiB minus the kernel's static reduction arrays (48 B), rounded
int attn_ref_max_ctx(int hd) { int n = 0; while (attn_ref_lds(n + 8, hd) <= ATTN_REF_DYN_LDS) n += 8; return n; }
// the > 64 KiB dynamic-LDS opt-in of a kernel: once per DEVICE (the attribute belongs to the device's code object), and a refusal is an error here, not a launch failure later
static unsigned long long g_attn_ref_optin_mask = 0;                       // bit d: device d has the attribute for both instantiations (<= 64 devices per process)
void attn_ref_prepare() {   // called by Engine::init / set_parity when parity mode is switched on -- never inside a stream capture (an attribute call there is refused)
    int dev = 0; HIP_CHECK(hipGetDevice(&dev));
    if (dev < 64 && (g_attn_ref_optin_mask >> dev & 1)) return;
    // (a request for the full 160 KiB is refused -- invalid argument -- because the kernels also have static LDS; rounds 3-4 asked for exactly that behind HIP_IGNORE, so the
    // opt-in never took effect and parity mode silently depended on staying below the 64 KiB default)
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_attn_ref<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_REF_DYN_LDS));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_attn_ref<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_REF_DYN_LDS));
    if (dev < 64) g_attn_ref_optin_mask |= 1ull << dev;
}
template <typename K> static void attn_ref_lds_optin(K kernel) {       // launchers reached without attn_ref_prepare (test hooks): best effort, as before
    int dev = 0; if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return; }
    if (dev < 64 && (g_attn_ref_optin_mask >> dev & 1)) return;
    HIP_IGNORE(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_REF_DYN_LDS));
}
void launch_attn_ref(const float *q, const __half *kcache, const __half *vcache, int N, int n_head, int hd, const int *n_past, int t_max, const Tables &tb, float *out, hipStream_t s) {
    note_kernel("k_attn_ref");
    attn_ref_lds_optin(&k_attn_ref<false>);
    hipLaunchKernelGGL(k_attn_ref<false>, dim3((unsigned)n_head, (unsigned)N), dim3(256), attn_ref_lds(t_max, hd), s, q, nullptr, nullptr, const_cast<__half *>(kcache), const_cast<__half *>(vcache),
                       n_head * hd, hd, n_past, nullptr, nullptr, tb, out);
}
// one query row: RoPE + cache append + attention in one launch (q, k, v: the raw projections; q is left unrotated)
void launch_attn_ref_fused(const float *q, const float *k, const float *v, __half *kcache, __half *vcache, int n_head, int hd, const int *n_past, int t_max, const float *cos_tab, const float *sin_tab,
                           const Tables &tb, float *out, hipStream_t s) {
    note_kernel("k_attn_ref");
    attn_ref_lds_optin(&k_attn_ref<true>);
    hipLaunchKernelGGL(k_attn_ref<true>, dim3((unsigned)n_head, 1), dim3(256), attn_ref_lds(t_max, hd), s, q, k, v, kcache, vcache, n_head * hd, hd, n_past, cos_tab, sin_tab, tb, out);
}

// =====================================================================================================================
// argmax (first maximum wins, like llama_sample_token_greedy) and small elementwise helpers
// =====================================================================================================================
constexpr int AM_BLOCKS = 64;
__device__ __forceinline__ void argmax_combine(float &best, int &bi, float ov, int oi) { if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; } }
__device__ __forceinline__ void argmax_wave(float &best, int &bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o); argmax_combine(best, bi, ov, oi); }
}
__global__ __launch_bounds__(256) void k_argmax_part(const float *__restrict__ x, int n, float *__restrict__ pv, int *__restrict__ pi) {
    if (MV_PIN_AT_ENTRY) asm volatile("" ::"s"(x), "s"(n), "s"(pv), "s"(pi));
    float best = -INFINITY; int bi = 0x7FFFFFFF;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += AM_BLOCKS * 256) { const float v = x[i]; if (v > best) { best = v; bi = i; } }
    __shared__ float sv[4]; __shared__ int si[4];
    argmax_wave(best, bi);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) { for (int w = 1; w < 4; w++) argmax_combine(best, bi, sv[w], si[w]); pv[blockIdx.x] = best; pi[blockIdx.x] = bi; }
}
__global__ __launch_bounds__(64) void k_argmax_final(const float *__restrict__ pv, const int *__restrict__ pi, int *__restrict__ out) {
    float best = pv[threadIdx.x]; int bi = pi[threadIdx.x];
    argmax_wave(best, bi);
    if (threadIdx.x == 0) *out = bi == 0x7FFFFFFF ? 0 : bi;
}
// (Round 5 measured argmax + advance as ONE launch -- last-arriving workgroup reduces the partial maxima and advances the position: 374.1 vs 374.4 tok/s, no difference;
// removed again, profiles/r05_experiments_not_adopted.md.)
// first maximum wins, like llama_sample_token_greedy.  `scratch` holds AM_BLOCKS floats + AM_BLOCKS ints.
void launch_argmax(const float *logits, int n, int *out, void *scratch, hipStream_t s) {
    note_kernel("k_argmax_part"); note_kernel("k_argmax_final");
    float *pv = static_cast<float *>(scratch); int *pi = reinterpret_cast<int *>(pv + AM_BLOCKS);
    hipLaunchKernelGGL(k_argmax_part, dim3(AM_BLOCKS), dim3(256), 0, s, logits, n, pv, pi);
    hipLaunchKernelGGL(k_argmax_final, dim3(1), dim3(64), 0, s, pv, pi, out);
}

__global__ void k_add_inplace(float *__restrict__ x, const float *__restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] + y[i];
}
void launch_add_inplace(float *x, const float *y, size_t n, hipStream_t s) { hipLaunchKernelGGL(k_add_inplace, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n); }

__global__ __launch_bounds__(256) void k_checksum(const unsigned *__restrict__ p, size_t n_words, unsigned long long *out) {
    unsigned long long s = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x) s += p[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, s);                      // integer sum: order does not matter
}
uint64_t device_checksum(const void *p, size_t bytes, hipStream_t s) {
    struct Word { unsigned long long *d = nullptr; ~Word() { if (d) HIP_IGNORE(hipFree(d)); } } w;   // freed on every path, also when a check below throws
    unsigned long long h = 0;
    HIP_CHECK(hipMalloc((void **)&w.d, 8));
    HIP_CHECK(hipMemsetAsync(w.d, 0, 8, s));
    hipLaunchKernelGGL(k_checksum, dim3(2048), dim3(256), 0, s, static_cast<const unsigned *>(p), bytes / 4, w.d);
    HIP_CHECK(hipMemcpyAsync(&h, w.d, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return (uint64_t)h;
}
// Fault injection for the native broadcast's bounded waits (MINIGPT4_DIST_TEST_STALL_MS, tests/test_gpu_serve.py): one lane keeps the stream busy for `ms` milliseconds
// of the 100 MHz constant clock -- what a collective whose peer died looks like to the host -- and then ENDS (at most 5 s: it can never hang the device).
__global__ void k_stall(unsigned ms) {
    const unsigned long long t0 = wall_clock64(), ticks = (unsigned long long)(ms > 5000u ? 5000u : ms) * 100000ull;
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
void launch_stall(unsigned ms, hipStream_t s) { hipLaunchKernelGGL(k_stall, dim3(1), dim3(1), 0, s, ms); }
__global__ void k_fill_u16(unsigned short *p, size_t n, unsigned short v) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
void launch_fill_u16(void *p, size_t n, unsigned short v, hipStream_t s) { hipLaunchKernelGGL(k_fill_u16, dim3(1024), dim3(256), 0, s, (unsigned short *)p, n, v); }
__global__ void k_set_int(int *p, int v) { *p = v; }
void launch_set_int(int *p, int v, hipStream_t s) { hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, s, p, v); }
// Batched decode epilogue, one workgroup per row: greedy argmax of the row's logits (first maximum wins), stored with the logits' owner slot; the
// conversation's position advances by one and the greedy token becomes its next input.
// Returns the greedy id in thread 0 (the other threads' value is meaningless).  KEEP = false: the sweep alone, no copy into the slot's row (k_draft_argmax).
template <bool KEEP = true>
__device__ __forceinline__ int batch_finish_row(const float *__restrict__ logits, int n_vocab, int r, int slot, float *__restrict__ slot_logits) {
    const float *x = logits + (size_t)r * n_vocab;
    float *keep = slot_logits + (size_t)slot * n_vocab;                   // the conversation's own copy (sampling with temp > 0, minigpt4_amd_get_logits)
    float best = -INFINITY; int bi = 0x7FFFFFFF;
    // 16 waves, 16-byte loads (a 256-thread scalar loop took 35 us for 32 000 logits: 125 dependent trips); every thread visits its indices in ascending order and
    // argmax_combine prefers the lower index, so ties resolve to the first maximum as before
    const int n4 = (n_vocab & 3) == 0 ? n_vocab >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += 1024) {
        const float4 v = reinterpret_cast<const float4 *>(x)[i]; if (KEEP) reinterpret_cast<float4 *>(keep)[i] = v;
        if (v.x > best) { best = v.x; bi = 4 * i; } if (v.y > best) { best = v.y; bi = 4 * i + 1; } if (v.z > best) { best = v.z; bi = 4 * i + 2; } if (v.w > best) { best = v.w; bi = 4 * i + 3; }
    }
    for (int i = 4 * n4 + threadIdx.x; i < n_vocab; i += 1024) { const float v = x[i]; if (KEEP) keep[i] = v; if (v > best) { best = v; bi = i; } }
    __shared__ float sv[16]; __shared__ int si[16];
    argmax_wave(best, bi);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) for (int w = 1; w < 16; w++) argmax_combine(best, bi, sv[w], si[w]);
    return bi == 0x7FFFFFFF ? 0 : bi;
}
__global__ __launch_bounds__(1024) void k_batch_finish(const float *__restrict__ logits, int n_vocab, const int *__restrict__ row_slot, int *__restrict__ n_past, int *__restrict__ argmax,
                                                      int *__restrict__ feed, float *__restrict__ slot_logits) {
    const int r = blockIdx.x, slot = row_slot[r];
    const int id = batch_finish_row(logits, n_vocab, r, slot, slot_logits);
    if (threadIdx.x == 0) { argmax[slot] = id; feed[slot] = id; n_past[slot] += 1; }
}
void launch_batch_finish(const float *logits, int n_vocab, int B, const int *row_slot, int *n_past, int *argmax, int *feed, float *slot_logits, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_finish, dim3((unsigned)B), dim3(1024), 0, s, logits, n_vocab, row_slot, n_past, argmax, feed, slot_logits);
}
// Verify pass epilogue (Engine::verify_draft), two launches in stream order.  tok[0 .. R) are the pass's rows (tok[0] = the conversation's greedy token, tok[1 ..] the draft).
// k_draft_argmax, one workgroup per row: res[1 + r] = the first argmax of logits row r (batch_finish_row's sweep without the copy).
// k_draft_finish, one workgroup: m = the number of leading draft tokens the pass's own rows chose (tok[i + 1] == res[1 + i] for every i < m); row m becomes the
// conversation's state -- its logits row, greedy and feed token res[1 + m], position p + 1 + m (n_past[slot] still holds p: the attention launches read it) -- and res[0] = m.
__global__ __launch_bounds__(1024) void k_draft_argmax(const float *__restrict__ logits, int n_vocab, int *__restrict__ res) {
    const int id = batch_finish_row<false>(logits, n_vocab, blockIdx.x, 0, nullptr);
    if (threadIdx.x == 0) res[1 + blockIdx.x] = id;
}
__global__ __launch_bounds__(1024) void k_draft_finish(const float *__restrict__ logits, int n_vocab, int R, const int *__restrict__ tok, const int *__restrict__ row_slot, int *__restrict__ n_past,
                                                      int *__restrict__ argmax, int *__restrict__ feed, float *__restrict__ slot_logits, int *__restrict__ res) {
    int m = 0;
    while (m < R - 1 && tok[m + 1] == res[1 + m]) m++;                    // every thread: R <= 8 words, all in cache
    const int slot = row_slot[0];
    const float *x = logits + (size_t)m * n_vocab;
    float *keep = slot_logits + (size_t)slot * n_vocab;
    for (int i = threadIdx.x; i < n_vocab; i += 1024) keep[i] = x[i];
    if (threadIdx.x == 0) { const int id = res[1 + m]; argmax[slot] = id; feed[slot] = id; n_past[slot] += 1 + m; res[0] = m; }
}
void launch_draft_finish(const float *logits, int n_vocab, int R, const int *tok, const int *row_slot, int *n_past, int *argmax, int *feed, float *slot_logits, int *res, hipStream_t s) {
    if (R < 1 || R > DRAFT_ROWS) throw HipError{hipErrorInvalidValue, "launch_draft_finish: row count out of range", __FILE__, __LINE__};
    note_kernel("k_draft_argmax"); note_kernel("k_draft_finish");
    hipLaunchKernelGGL(k_draft_argmax, dim3((unsigned)R), dim3(1024), 0, s, logits, n_vocab, res);
    hipLaunchKernelGGL(k_draft_finish, dim3(1), dim3(1024), 0, s, logits, n_vocab, R, tok, row_slot, n_past, argmax, feed, slot_logits, res);
}
// verify pass prologue: the host's view of the conversation's position, once (every row of the pass derives its own from it)
__global__ void k_draft_begin(int *__restrict__ n_past, const int *__restrict__ row_slot, const int *__restrict__ row_pos) { n_past[row_slot[0]] = row_pos[0]; }
void launch_draft_begin(int *n_past, const int *row_slot, const int *row_pos, hipStream_t s) { hipLaunchKernelGGL(k_draft_begin, dim3(1), dim3(1), 0, s, n_past, row_slot, row_pos); }
// Verify pass of several conversations (Engine::verify_draft_batch): N packed rows in consecutive groups, one group per conversation, all slots distinct -- so a group
// starts at row 0 and wherever the slot differs from the row before, and nothing but row_slot / row_pos describes the grouping.
// k_mdraft_begin (replaces k_draft_begin): n_past[slot] = the position of the group's first row.
// Epilogue, two launches in stream order over the result block res = m [ATTN_MDRAFT_ROWS] | row_greedy [ATTN_MDRAFT_ROWS]:
//   k_draft_argmax over the N rows, writing row_greedy (it is handed res + ATTN_MDRAFT_ROWS - 1: its entry 1 + t is row_greedy[t]);
//   k_draft_finish_batch, one workgroup per packed row of which those on a group's first row t0 work: R = the group's rows, m = the number of leading draft tokens with
//   tok[t0 + i + 1] == row_greedy[t0 + i]; logits row t0 + m becomes the conversation's, argmax = feed = row_greedy[t0 + m], n_past += 1 + m, m[t0] = m.  The others
//   write m[t] = -1 and leave.  Conversations not in the pass are not touched.
__global__ void k_mdraft_begin(int *__restrict__ n_past, const int *__restrict__ row_slot, const int *__restrict__ row_pos, int N) {
    const int t = threadIdx.x;
    if (t < N && (t == 0 || row_slot[t] != row_slot[t - 1])) n_past[row_slot[t]] = row_pos[t];
}
void launch_mdraft_begin(int *n_past, const int *row_slot, const int *row_pos, int N, hipStream_t s) {
    if (N < 1 || N > ATTN_MDRAFT_ROWS) throw HipError{hipErrorInvalidValue, "launch_mdraft_begin: row count out of range", __FILE__, __LINE__};
    hipLaunchKernelGGL(k_mdraft_begin, dim3(1), dim3(ATTN_MDRAFT_ROWS), 0, s, n_past, row_slot, row_pos, N);
}
__global__ __launch_bounds__(1024) void k_draft_finish_batch(const float *__restrict__ logits, int n_vocab, int N, const int *__restrict__ tok, const int *__restrict__ row_slot,
                                                            int *__restrict__ n_past, int *__restrict__ argmax, int *__restrict__ feed, float *__restrict__ slot_logits, int *__restrict__ res) {
    const int t0 = blockIdx.x, slot = row_slot[t0];
    if (t0 > 0 && row_slot[t0 - 1] == slot) { if (threadIdx.x == 0) res[t0] = -1; return; }   // not a group's first row (uniform over the workgroup)
    int R = 1;
    while (R < DRAFT_ROWS && t0 + R < N && row_slot[t0 + R] == slot) R++;
    const int *g = res + ATTN_MDRAFT_ROWS + t0;                            // the group's greedy ids (k_draft_argmax, the launch before)
    int m = 0;
    while (m < R - 1 && tok[t0 + m + 1] == g[m]) m++;                      // every thread: R <= 8 words, all in cache
    const float *x = logits + (size_t)(t0 + m) * n_vocab;
    float *keep = slot_logits + (size_t)slot * n_vocab;
    for (int i = threadIdx.x; i < n_vocab; i += 1024) keep[i] = x[i];
    if (threadIdx.x == 0) { const int id = g[m]; argmax[slot] = id; feed[slot] = id; n_past[slot] += 1 + m; res[t0] = m; }
}
void launch_draft_finish_batch(const float *logits, int n_vocab, int N, const int *tok, const int *row_slot, int *n_past, int *argmax, int *feed, float *slot_logits, int *res, hipStream_t s) {
    if (N < 1 || N > ATTN_MDRAFT_ROWS) throw HipError{hipErrorInvalidValue, "launch_draft_finish_batch: row count out of range", __FILE__, __LINE__};
    note_kernel("k_draft_argmax"); note_kernel("k_draft_finish_batch");
    hipLaunchKernelGGL(k_draft_argmax, dim3((unsigned)N), dim3(1024), 0, s, logits, n_vocab, res + ATTN_MDRAFT_ROWS - 1);
    hipLaunchKernelGGL(k_draft_finish_batch, dim3((unsigned)N), dim3(1024), 0, s, logits, n_vocab, N, tok, row_slot, n_past, argmax, feed, slot_logits, res);
}
// Packed prompt chunk epilogue (Engine::prefill_batch): row r of `logits` is the last row of conversation fin[2 r]; its position becomes fin[2 r + 1] (set, not
// advanced), its greedy id and feed token as k_batch_finish writes them.
__global__ __launch_bounds__(1024) void k_seg_finish(const float *__restrict__ logits, int n_vocab, const int *__restrict__ fin, int *__restrict__ n_past, int *__restrict__ argmax,
                                                    int *__restrict__ feed, float *__restrict__ slot_logits) {
    const int r = blockIdx.x, slot = fin[2 * r];
    const int id = batch_finish_row(logits, n_vocab, r, slot, slot_logits);
    if (threadIdx.x == 0) { argmax[slot] = id; feed[slot] = id; n_past[slot] = fin[2 * r + 1]; }
}
void launch_seg_finish(const float *logits, int n_vocab, int B, const int *fin, int *n_past, int *argmax, int *feed, float *slot_logits, hipStream_t s) {
    note_kernel("k_seg_finish");
    hipLaunchKernelGGL(k_seg_finish, dim3((unsigned)B), dim3(1024), 0, s, logits, n_vocab, fin, n_past, argmax, feed, slot_logits);
}
// dst[r] = src[idx[r]] (rows of E floats)
__global__ void k_gather_rows(const float *__restrict__ src, const int *__restrict__ idx, int E, float *__restrict__ dst) {
    const float *a = src + (size_t)idx[blockIdx.x] * E;
    float *b = dst + (size_t)blockIdx.x * E;
    for (int i = threadIdx.x; i < E; i += blockDim.x) b[i] = a[i];
}
void launch_gather_rows(const float *src, const int *idx, int n, int E, float *dst, hipStream_t s) {
    note_kernel("k_gather_rows");
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)n), dim3(256), 0, s, src, idx, E, dst);
}
// The row as its sweeps see it, shared by k_logprob_rows and k_topn_rows (which must report the same bits): scalar head [0, head), 16-byte body, scalar tail [tail0, n).
struct RowSpan { const float *x; const float4 *x4; int head, n4, tail0, n; };
__device__ __forceinline__ RowSpan row_span(const float *x, int n_vocab) {
    RowSpan s; s.x = x; s.n = n_vocab;
    s.head = min(n_vocab, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 2);
    s.n4 = (n_vocab - s.head) >> 2; s.tail0 = s.head + 4 * s.n4;
    s.x4 = reinterpret_cast<const float4 *>(x + s.head);
    return s;
}
// one sweep of a 256-thread workgroup: f(value, index) for every element, a thread's indices in ascending order
template <typename F> __device__ __forceinline__ void row_sweep(const RowSpan &s, int tid, F f) {
    if (tid < s.head) f(s.x[tid], tid);
    for (int i = tid; i < s.n4; i += 256) { const float4 v = s.x4[i]; const int b = s.head + 4 * i; f(v.x, b); f(v.y, b + 1); f(v.z, b + 2); f(v.w, b + 3); }
    if (s.tail0 + tid < s.n) f(s.x[s.tail0 + tid], s.tail0 + tid);
}
// the row's maximum and its first index, in every thread (sv, si: 4 entries of LDS)
__device__ __forceinline__ void row_max_first(const RowSpan &s, int tid, float *sv, int *si, float &best, int &bi) {
    best = -INFINITY; bi = 0x7FFFFFFF;
    row_sweep(s, tid, [&](float v, int i) { argmax_combine(best, bi, v, i); });
    argmax_wave(best, bi);
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    best = sv[0]; bi = si[0];
    for (int w = 1; w < 4; w++) argmax_combine(best, bi, sv[w], si[w]);   // every thread: the row's maximum, uniformly
}
// sum of exp(x - best) over the row, in every thread (ss: 4 entries of LDS): per-thread sums in sweep order, xor tree per wave, (w0 + w1) + (w2 + w3)
__device__ __forceinline__ float row_sum_exp(const RowSpan &s, int tid, float best, float *ss) {
    float sum = 0.0f;
    row_sweep(s, tid, [&](float v, int) { sum += expf(v - best); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((tid & 63) == 0) ss[tid >> 6] = sum;
    __syncthreads();
    return (ss[0] + ss[1]) + (ss[2] + ss[3]);
}
// Scoring (Engine::score_tokens): one workgroup per logits row.  Sweep 1: the row's maximum and its first index; sweep 2: sum of exp(x - max) (the row was just
// written, both sweeps hit L2).  logprob = (x[target] - max) - log(sum): the maximum's own term is exp(0) = 1, so sum >= 1 and no single exp is ever passed to log.
// Rows start at logits + r * ld with any ld >= n_vocab (32001 floats: not 16-byte aligned from row 1 on), so each row takes its own scalar head up to the first
// aligned address, 16-byte loads over the body and a scalar tail; every element carries its index and argmax_combine prefers the lower one, whatever order a thread meets them in.
__global__ __launch_bounds__(256) void k_logprob_rows(const float *__restrict__ logits, int ld, int n_vocab, const int *__restrict__ targets, float *__restrict__ logprob,
                                                      int *__restrict__ greedy, float *__restrict__ greedy_logprob) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const float *x = logits + (size_t)r * ld;
    const RowSpan sp = row_span(x, n_vocab);
    __shared__ float sv[4]; __shared__ int si[4]; __shared__ float ss[4];
    float best; int bi;
    row_max_first(sp, tid, sv, si, best, bi);
    const float sum = row_sum_exp(sp, tid, best, ss);
    if (tid == 0) {
        const float lse = logf(sum);
        const int t = targets[r];
        greedy[r] = bi == 0x7FFFFFFF ? 0 : bi;
        greedy_logprob[r] = -lse;
        logprob[r] = t >= 0 && t < n_vocab ? (x[t] - best) - lse : 0.0f;
    }
}
void launch_logprob_rows(const float *logits, int ld, int n_vocab, int rows, const int *targets, float *logprob, int *greedy, float *greedy_logprob, hipStream_t s) {
    note_kernel("k_logprob_rows");
    hipLaunchKernelGGL(k_logprob_rows, dim3((unsigned)rows), dim3(256), 0, s, logits, ld, n_vocab, targets, logprob, greedy, greedy_logprob);
}
// Top-N alternatives (Engine::top_logprobs, score_tokens_top, decode_batch's report): one workgroup per logits row, the first top_n tokens in the order "logit
// descending, equal logits by ascending id" (sampler.cpp's sort_desc_by_logit), their log-softmax -- the bits k_logprob_rows reports: row_max_first / row_sum_exp
// and the same (x - max) - log(sum) -- and the rank of targets[r] in that order.  The selection works on an order-preserving 32-bit key (-0 canonicalised, so -0 and
// +0 tie) and never sorts the row.  SWEEPS over the row: 7 at the most, whatever top_n and whatever the data -- maximum, sum of exponentials, three histogram levels
// (11 + 11 + 10 key bits in 8 KB of LDS) that find the exact key T of the top_n-th token, one collecting sweep (keys above T: fewer than top_n; keys equal to T:
// the first 192 that arrive; the target's rank), and, only when more than 192 keys equal T, a scan in id order that takes the lowest ids among them and stops when
// it has them (7-level or all-equal rows; at most one more sweep).  An all-equal row does not serialise on one LDS word: a histogram add peels the lanes that
// share the first active lane's bin into one atomic, the tie list takes one atomic per wave.  The <= 256 candidates are then placed by counting predecessors.
// Logits are finite (NaN / infinities: unspecified).  Nothing beyond n_vocab floats of a row is read.
__device__ __forceinline__ unsigned topn_key(float v) {
    const unsigned u = __float_as_uint(v == 0.0f ? 0.0f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);                       // ascending in the float's value
}
__device__ __forceinline__ void topn_hist_add(unsigned *hist, bool take, unsigned bin, int lane) {
    if (take) {
        const unsigned long long m = __ballot(1);
        const int leader = __ffsll((long long)m) - 1;
        const unsigned b0 = (unsigned)__shfl((int)bin, leader);
        const unsigned long long same = __ballot(bin == b0);
        if (bin != b0) atomicAdd(&hist[bin], 1u);
        else if (lane == leader) atomicAdd(&hist[b0], (unsigned)__popcll(same));
    }
}
__device__ __forceinline__ unsigned topn_wave_scan(unsigned v, int lane) {   // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = (unsigned)__shfl_up((int)v, o); if (lane >= o) v += t; }
    return v;
}
// hist[0, 256 per): the bin b, counted from the top, with above < k <= above + hist[b] (above = the count in the bins over b); uniform in every thread
__device__ __forceinline__ void topn_select(const unsigned *hist, int per, unsigned k, int tid, unsigned *sw, unsigned *sres, unsigned &bin, unsigned &above) {
    const int nb = per * 256, lane = tid & 63, top = nb - 1 - tid * per;      // this thread's bins: top, top - 1, ..., top - per + 1
    unsigned own = 0;
    for (int j = 0; j < per; j++) own += hist[top - j];
    const unsigned inc = topn_wave_scan(own, lane);
    if (lane == 63) sw[tid >> 6] = inc;
    __syncthreads();
    unsigned before = inc - own;
    for (int w = 0; w < (tid >> 6); w++) before += sw[w];
    if (before < k && k <= before + own) {                                    // exactly one thread (the bins hold at least k)
        unsigned a = before;
        for (int j = 0; j < per; j++) { const unsigned h = hist[top - j]; if (k <= a + h) { sres[0] = (unsigned)(top - j); sres[1] = a; break; } a += h; }
    }
    __syncthreads();
    bin = sres[0]; above = sres[1];
    __syncthreads();
}
__global__ __launch_bounds__(256) void k_topn_rows(const float *__restrict__ logits, int ld, int n_vocab, const int *__restrict__ row_index, int top_n,
                                                   const int *__restrict__ targets, int *__restrict__ ids, float *__restrict__ logprobs, int *__restrict__ rank,
                                                   float *__restrict__ target_logprob) {
    constexpr int GT = TOPN_MAX, TIES = 256 - TOPN_MAX;                      // candidate list: keys above T in [0, GT), keys equal to T in [GT, 256)
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const float *x = logits + (size_t)(row_index ? row_index[r] : r) * ld;
    const RowSpan sp = row_span(x, n_vocab);
    __shared__ float sv[4]; __shared__ int si[4]; __shared__ float ss[4];
    __shared__ unsigned hist[2048], sw[4], sres[2], ckey[256];
    __shared__ int cid[256], cnt[3];                                          // cnt: keys above T, keys equal to T, the target's rank
    if (tid < 3) cnt[tid] = 0;
    float best; int bi;
    row_max_first(sp, tid, sv, si, best, bi);
    const float lse = logf(row_sum_exp(sp, tid, best, ss));
    // the key of the top_n-th token: three levels, each a histogram of the keys that share the prefix found so far
    unsigned b1, b2, b3, a1, a2, a3;
    for (int i = tid; i < 2048; i += 256) hist[i] = 0;
    __syncthreads();
    row_sweep(sp, tid, [&](float v, int) { topn_hist_add(hist, true, topn_key(v) >> 21, lane); });
    __syncthreads();
    topn_select(hist, 8, (unsigned)top_n, tid, sw, sres, b1, a1);
    for (int i = tid; i < 2048; i += 256) hist[i] = 0;
    __syncthreads();
    row_sweep(sp, tid, [&](float v, int) { const unsigned k = topn_key(v); topn_hist_add(hist, (k >> 21) == b1, (k >> 10) & 2047u, lane); });
    __syncthreads();
    topn_select(hist, 8, (unsigned)top_n - a1, tid, sw, sres, b2, a2);
    const unsigned p2 = (b1 << 11) | b2;
    for (int i = tid; i < 1024; i += 256) hist[i] = 0;
    __syncthreads();
    row_sweep(sp, tid, [&](float v, int) { const unsigned k = topn_key(v); topn_hist_add(hist, (k >> 10) == p2, k & 1023u, lane); });
    __syncthreads();
    topn_select(hist, 4, (unsigned)top_n - a1 - a2, tid, sw, sres, b3, a3);
    const unsigned T = (p2 << 10) | b3;
    const int n_gt = (int)(a1 + a2 + a3), need = top_n - n_gt;                // n_gt < top_n keys lie above T, at least `need` >= 1 equal it
    // the collecting sweep
    const int t = targets[r];
    const bool has_t = t >= 0 && t < n_vocab;
    const unsigned tkey = has_t ? topn_key(x[t]) : 0u;
    int before_t = 0;
    row_sweep(sp, tid, [&](float v, int i) {
        const unsigned k = topn_key(v);
        if (has_t) before_t += (k > tkey || (k == tkey && i < t)) ? 1 : 0;
        if (k > T) {
            const int p = atomicAdd(&cnt[0], 1);
            if (p < GT) { ckey[p] = k; cid[p] = i; }
        } else if (k == T) {
            const unsigned long long m = __ballot(1);
            const int leader = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&cnt[1], (int)__popcll(m));
            const int p = __shfl(base, leader) + (int)__popcll(m & ((1ull << lane) - 1ull));
            if (p < TIES) { ckey[GT + p] = k; cid[GT + p] = i; }
        }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before_t += __shfl_xor(before_t, o);
    if (lane == 0 && before_t) atomicAdd(&cnt[2], before_t);
    __syncthreads();
    int n_tie = cnt[1];
    if (n_tie > TIES) {   // (uniform) too many keys equal T to have been listed: the lowest `need` ids among them, 1024 ids per step, in id order
        int taken = 0;
        for (int base = 0; base < n_vocab && taken < need; base += 1024) {
            const int i0 = base + 4 * tid;
            unsigned m4 = 0;
            for (int j = 0; j < 4; j++) if (i0 + j < n_vocab && topn_key(x[i0 + j]) == T) m4 |= 1u << j;
            const unsigned c = (unsigned)__popc(m4), inc = topn_wave_scan(c, lane);
            if (lane == 63) sw[tid >> 6] = inc;
            __syncthreads();
            int at = taken + (int)(inc - c);
            for (int w = 0; w < (tid >> 6); w++) at += (int)sw[w];
            for (int j = 0; j < 4; j++) if ((m4 >> j) & 1u) { if (at < need) { ckey[GT + at] = T; cid[GT + at] = i0 + j; } at++; }
            taken += (int)(sw[0] + sw[1] + sw[2] + sw[3]);
            __syncthreads();
        }
        n_tie = need;
    }
    __syncthreads();
    // placement: a key above T goes behind the keys above it (equal ones by id); a key equal to T behind all of those and the lower ids of its own kind
    const bool is_gt = tid < n_gt, is_tie = tid >= GT && tid < GT + n_tie;
    if (is_gt || is_tie) {
        const unsigned mk = ckey[tid]; const int mi = cid[tid];
        int pos = is_gt ? 0 : n_gt;
        if (is_gt) { for (int c = 0; c < n_gt; c++) pos += (ckey[c] > mk || (ckey[c] == mk && cid[c] < mi)) ? 1 : 0; }
        else for (int c = GT; c < GT + n_tie; c++) pos += cid[c] < mi ? 1 : 0;
        if (pos < top_n) { ids[(size_t)r * top_n + pos] = mi; logprobs[(size_t)r * top_n + pos] = (x[mi] - best) - lse; }
    }
    if (tid == 0) { rank[r] = has_t ? cnt[2] : -1; target_logprob[r] = has_t ? (x[t] - best) - lse : 0.0f; }
}
bool launch_topn_rows(const float *logits, int ld, int n_vocab, int rows, const int *row_index, int top_n, const int *targets, int *ids, float *logprobs, int *rank,
                      float *target_logprob, hipStream_t s) {
    if (rows < 1 || n_vocab < 1 || ld < n_vocab || top_n < 1 || top_n > TOPN_MAX || top_n > n_vocab) { set_last_error("launch_topn_rows: shape out of range"); return false; }
    note_kernel("k_topn_rows");
    hipLaunchKernelGGL(k_topn_rows, dim3((unsigned)rows), dim3(256), 0, s, logits, ld, n_vocab, row_index, top_n, targets, ids, logprobs, rank, target_logprob);
    return true;
}
// One beam-search step's decision (Engine::beam_search; beam.hpp holds the rule and its arithmetic, shared with the host), ONE workgroup of BEAM_MAX * BEAM_CAND_MAX = 128
// threads, one launch per step.  Thread j owns candidate j = beam * C + c of the [W][C] ids / log-probabilities k_topn_rows just wrote: its score is one fp32 add, its rank
// the number of live candidates that sort before it (beam_rank_of -- the counting placement of k_topn_rows; no sort, no atomics), order[rank] = j.  Thread 0 then walks the
// ranking (beam_walk) and writes the result block, the next step's scores and the row tokens of the weight pass that follows in the stream -- no host round trip between
// the logits of step t and the pass of step t + 1; the host reads *res through pinned memory while that pass runs.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): 22 VGPRs, 93 SGPRs, no scratch, 1712 bytes of LDS, occupancy 8 waves per SIMD.
__global__ __launch_bounds__(BEAM_MAX * BEAM_CAND_MAX) void k_beam_select(const int *__restrict__ ids, const float *__restrict__ logprobs, float *scores, unsigned live, int W, int C,
                                                                         int eos, int n_vocab, BeamStep *__restrict__ res, int *__restrict__ row_tok) {
    constexpr int N = BEAM_MAX * BEAM_CAND_MAX;
    __shared__ float cand[N]; __shared__ int cid[N], order[N]; __shared__ BeamStep st;
    const int j = threadIdx.x, n = W * C;
    const bool mine = j < n && ((live >> (j / C)) & 1u);
    order[j] = -1;
    if (j < n) { cand[j] = beam_score(scores[j / C], logprobs[j]); cid[j] = ids[j]; }
    __syncthreads();
    if (mine) order[beam_rank_of(j, cand, W, C, live)] = j;
    __syncthreads();
    if (j == 0) beam_walk(order, __popc(live & ((1u << W) - 1u)) * C, cid, cand, W, C, eos, st);
    __syncthreads();
    if (j < (int)(sizeof(BeamStep) / 4)) reinterpret_cast<int *>(res)[j] = reinterpret_cast<const int *>(&st)[j];
    if (j < W) { scores[j] = st.score[j]; const int t = st.tok[j]; row_tok[j] = t >= 0 && t < n_vocab ? t : 0; }
}
bool launch_beam_select(const int *ids, const float *logprobs, float *scores, unsigned live, int W, int C, int eos, int n_vocab, BeamStep *res, int *row_tok, hipStream_t s) {
    if (!ids || !logprobs || !scores || !res || !row_tok || W < 2 || W > BEAM_MAX || C < 1 || C > BEAM_CAND_MAX || n_vocab < 1 || !(live & ((1u << W) - 1u))) {
        set_last_error("launch_beam_select: shape out of range"); return false;
    }
    note_kernel("k_beam_select");
    hipLaunchKernelGGL(k_beam_select, dim3(1), dim3(BEAM_MAX * BEAM_CAND_MAX), 0, s, ids, logprobs, scores, live, W, C, eos, n_vocab, res, row_tok);
    return true;
}
#include "pick_row.hpp"
// Penalised greedy pick (Engine::pen_pick), one workgroup of 256 per listed conversation, one launch for all of them.  rows[r] names the logits row, the conversation's
// table (penalty.hpp: the distinct ids its repetition / frequency / presence penalties and its logit bias touch) and the factors.  pick_row.hpp holds the walk (the table
// ids marked in ONE bitmap in LDS, the sweep over the unmarked ids, the table loop through pen_value) and the greedy tail; "larger value, then smaller id" over both sets
// is the first maximum of the transformed row.  The row is read in place and never written: whoever reads logits_ afterwards (minigpt4_amd_get_logits, scoring, top-N)
// sees raw logits.  picked[r] = the id (0 for a row without a comparable value); adjusted (may be null): the value of every table entry, at the entry's index (test hook).
// LDS, all dynamic: (n_vocab + 31) / 32 bitmap words rounded up to 4, then 4 floats and 4 ints of reduction scratch.
__global__ __launch_bounds__(256) void k_pen_pick(const float *__restrict__ logits, int ld, int n_vocab, const PenRow *__restrict__ rows, const PenEntry *__restrict__ table,
                                                  int *__restrict__ picked, float *__restrict__ adjusted) {
    extern __shared__ __attribute__((aligned(16))) unsigned pen_lds[];
    const int id = pick_greedy<false>(logits, ld, n_vocab, rows[blockIdx.x], table, nullptr, adjusted, 0, pen_lds, threadIdx.x);
    if (threadIdx.x == 0) picked[blockIdx.x] = id;
}
bool launch_pen_pick(const float *logits, int ld, int n_vocab, int n_rows, const PenRow *rows, const PenEntry *table, int *picked, float *adjusted, hipStream_t s) {
    const size_t lds = ((size_t)(((n_vocab + 31) / 32 + 3) & ~3) + 8) * 4;
    if (n_rows < 1 || n_vocab < 1 || ld < n_vocab || lds > 64 * 1024) { set_last_error("launch_pen_pick: shape out of range"); return false; }
    note_kernel("k_pen_pick");
    hipLaunchKernelGGL(k_pen_pick, dim3((unsigned)n_rows), dim3(256), lds, s, logits, ld, n_vocab, rows, table, picked, adjusted);
    return true;
}
// Constrained decoding, the index (Engine::constraint_compile; constraint.hpp): index[s][W] = the bitmap of the token ids a conversation in DFA state s may emit, built once
// per compiled pattern.  One workgroup of 256 per state, a lane walks one token's bytes (vocab[off[i] .. off[i + 1]), unsigned) from s through constraint_walk -- the
// function the host walks picked tokens with --, a wave takes 64 consecutive ids and one lane stores its ballot as two words: no atomics, every word of the row written once.
// Bit i: i >= 3, the piece is not empty and the walk does not end in state 0; i == 2 (EOS) iff s accepts; ids 0, 1, ids >= n_vocab and all of row 0: zero.
// W = (n_vocab + 31) / 32 rounded up to 4, so 32 W is a multiple of 128 and every wave's 64 ids lie inside the row.  Reads: off[0 .. n_vocab], vocab below off[n_vocab],
// trans below S * 256 (its entries are < S: the compiler's table; the test hook checks a given one).  No LDS.
__global__ __launch_bounds__(256) void k_constrain_index(const unsigned char *__restrict__ vocab, const int *__restrict__ off, int n_vocab, const uint16_t *__restrict__ trans,
                                                         const unsigned *__restrict__ accept, int W, unsigned *__restrict__ index) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const bool accepting = s != CONSTRAINT_DEAD && ((accept[s >> 5] >> (s & 31)) & 1u);
    unsigned *row = index + (size_t)s * W;
    for (int i0 = (tid >> 6) * 64; i0 < 32 * W; i0 += 256) {                 // wave-uniform bounds: all 64 lanes vote
        const int i = i0 + (tid & 63);
        bool ok = false;
        if (s != CONSTRAINT_DEAD && i < n_vocab) {
            if (i == CONSTRAINT_EOS) ok = accepting;
            else if (i > CONSTRAINT_EOS) { const int a = off[i], n = off[i + 1] - a; ok = n > 0 && constraint_walk(trans, s, vocab + a, n) != CONSTRAINT_DEAD; }
        }
        const unsigned long long votes = __ballot(ok);
        if ((tid & 63) == 0) { row[i0 >> 5] = (unsigned)votes; row[(i0 >> 5) + 1] = (unsigned)(votes >> 32); }
    }
}
bool launch_constrain_index(const unsigned char *vocab, const int *off, int n_vocab, const uint16_t *trans, const unsigned *accept, int n_states, unsigned *index, hipStream_t s) {
    if (!vocab || !off || !trans || !accept || !index || n_vocab < 1 || n_states < 2 || n_states > CONSTRAINT_MAX_STATES) { set_last_error("launch_constrain_index: shape out of range"); return false; }
    note_kernel("k_constrain_index");
    hipLaunchKernelGGL(k_constrain_index, dim3((unsigned)n_states), dim3(256), 0, s, vocab, off, n_vocab, trans, accept, constraint_words(n_vocab), index);
    return true;
}
// Constrained greedy pick (Engine::con_pick), one workgroup of 256 per constrained conversation, one launch for all of them: k_pen_pick's body (pick_row.hpp) with the
// allowed bitmap.  rows[r] names the logits row, the address of index[state] (constraint_words(n_vocab) words; null: every id) and -- pen.n > 0 -- the conversation's
// penalty table and factors.  out[r] = the FIRST maximum of the transformed row over the allowed ids (larger value, then lower id; -0 == +0; an allowed id at -infinity can
// still win among -infinities; NaN never wins).  No allowed id: out[r] = CONSTRAINT_EOS | CONSTRAIN_STUCK.  The logits are read in place and never written.  LDS, all
// dynamic: 2 * constraint_words(n_vocab) bitmap words, then 4 floats and 4 ints of reduction scratch (8 KB at 32 001 ids); the launch refuses a vocabulary whose two
// bitmaps exceed 64 KB (n_vocab above 261 000).
__global__ __launch_bounds__(256) void k_constrain_pick(const float *__restrict__ logits, int ld, int n_vocab, const ConRow *__restrict__ rows, const PenEntry *__restrict__ table,
                                                        int *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned con_lds[];
    const ConRow cr = rows[blockIdx.x];
    const int id = pick_greedy<true>(logits, ld, n_vocab, cr.pen, table, cr.allowed, nullptr, CONSTRAINT_EOS | CONSTRAIN_STUCK, con_lds, threadIdx.x);
    if (threadIdx.x == 0) out[blockIdx.x] = id;
}
bool launch_constrain_pick(const float *logits, int ld, int n_vocab, int n_rows, const ConRow *rows, const PenEntry *table, int *out, hipStream_t s) {
    const size_t lds = ((size_t)2 * constraint_words(n_vocab) + 8) * 4;
    if (!logits || !rows || !out || n_rows < 1 || n_vocab < 1 || ld < n_vocab || lds > 64 * 1024) { set_last_error("launch_constrain_pick: shape out of range"); return false; }
    note_kernel("k_constrain_pick");
    hipLaunchKernelGGL(k_constrain_pick, dim3((unsigned)n_rows), dim3(256), lds, s, logits, ld, n_vocab, rows, table, out);
    return true;
}
// Guided decoding (Engine::decode_guided / guided_logits; minigpt4_amd.h states the rule), one workgroup of 256 per pair, one launch for all pairs of a call.  A pair names
// two logits rows, b (the guided conversation) and g (the guidance one), and a scale.  Sweeps: the maxima of the two rows and the two sums of exponentials through
// row_max_first / row_sum_exp -- so lb = (b - max b) - log(sum) and lg are the bits k_logprob_rows / k_topn_rows report for the same row at the same address -- and ONE mixing
// sweep: d = lb - lg, t = scale * d, m = lg + t, each rounded to fp32 on its own, carried into the first argmax by argmax_combine and stored to mixed[pair][n_vocab] only when
// a buffer is given.  The mixing sweep walks b's span (scalar head, 16-byte body, scalar tail); the two rows rarely share an alignment (32 001-float rows), so g and the
// output are addressed per element -- the rows were just written by the output mat-vec and sit in L2.  Every element's value depends on its own index only, whatever thread
// meets it.  Exact consequences: scale == 0 gives m == lg, b == g gives m == lb (d = +0, and lb is never -0: the maximum's term is +0 - log(sum >= 1)).
// pick[pair] = the first maximum of m (lowest id among equal values, -0 == +0), pick_val[pair] = m[pick]; row_tok (may be null): the pick goes straight into entries
// pos_tok and neg_tok (those >= 0) -- the row tokens of the weight pass that follows in the stream, as k_beam_select writes them.  Logits are finite (NaN / infinities:
// unspecified).  Nothing beyond n_vocab floats of a row is read; the rows are never written.  No atomics, no LDS beyond 32 words of reduction scratch.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): 42 VGPRs, 66 SGPRs, no scratch, 128 bytes of LDS, occupancy 8 waves per SIMD.
__global__ __launch_bounds__(256) void k_guide_rows(const float *__restrict__ logits, int ld, int n_vocab, const GuidePair *__restrict__ pairs, float *__restrict__ mixed,
                                                    int *__restrict__ pick, float *__restrict__ pick_val, int *__restrict__ row_tok) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const GuidePair gp = pairs[r];
    const float *b = logits + (size_t)gp.pos_row * ld, *g = logits + (size_t)gp.neg_row * ld;
    const RowSpan sb = row_span(b, n_vocab), sg = row_span(g, n_vocab);
    __shared__ float sv[3][4], ss[2][4]; __shared__ int si[3][4];              // one set per reduction: no word is written while another wave may still read it
    float max_b, max_g; int at_b, at_g;
    row_max_first(sb, tid, sv[0], si[0], max_b, at_b);
    row_max_first(sg, tid, sv[1], si[1], max_g, at_g);
    const float lse_b = logf(row_sum_exp(sb, tid, max_b, ss[0])), lse_g = logf(row_sum_exp(sg, tid, max_g, ss[1]));
    float *out = mixed ? mixed + (size_t)r * n_vocab : nullptr;
    const float scale = gp.scale;
    float best = -INFINITY; int bi = 0x7FFFFFFF;
    row_sweep(sb, tid, [&](float v, int i) {
        const float lb = __fsub_rn(__fsub_rn(v, max_b), lse_b), lg = __fsub_rn(__fsub_rn(g[i], max_g), lse_g);
        const float m = __fadd_rn(lg, __fmul_rn(scale, __fsub_rn(lb, lg)));
        if (out) out[i] = m;
        argmax_combine(best, bi, m, i);
    });
    argmax_wave(best, bi);
    if ((tid & 63) == 0) { sv[2][tid >> 6] = best; si[2][tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) argmax_combine(best, bi, sv[2][w], si[2][w]);
        const int id = bi == 0x7FFFFFFF ? 0 : bi;
        pick[r] = id; pick_val[r] = best;
        if (row_tok) { if (gp.pos_tok >= 0) row_tok[gp.pos_tok] = id; if (gp.neg_tok >= 0) row_tok[gp.neg_tok] = id; }
    }
}
bool launch_guide_rows(const float *logits, int ld, int n_vocab, int n_pairs, const GuidePair *pairs, float *mixed, int *pick, float *pick_val, int *row_tok, hipStream_t s) {
    if (!logits || !pairs || !pick || !pick_val || n_pairs < 1 || n_pairs > GUIDE_MAX || n_vocab < 1 || ld < n_vocab) { set_last_error("launch_guide_rows: shape out of range"); return false; }
    note_kernel("k_guide_rows");
    hipLaunchKernelGGL(k_guide_rows, dim3((unsigned)n_pairs), dim3(256), 0, s, logits, ld, n_vocab, pairs, mixed, pick, pick_val, row_tok);
    return true;
}
// Sampled decode step (Engine::decode_batch_sampled / sampled_candidates; sampling.hpp holds the generator and the rule's arithmetic, shared with the host), one workgroup
// of 256 per listed conversation, one launch for all of them.  rows[r] names the logits row, the conversation's penalty table and factors (as k_pen_pick takes them), the
// allowed bitmap of its constraint state (as k_constrain_pick takes it; null: every id), temp / top_k / top_p, the generator's (seed, draws) and the entry of the weight
// pass's row tokens that takes the pick (-1: none).  The row the rule sees -- bias and penalties, then the constraint -- is never materialised: pick_row.hpp's walk (the
// greedy picks' own) feeds every participating id, from the row sweep or from the table, into the same histograms and lists.  The selection is k_topn_rows': the same order-preserving key (topn_key), the same three histogram levels (11 + 11 + 10 bits)
// for the key T of the k-th participating id (k = min(top_k, participating ids)), the same collecting sweep (keys above T: fewer than k; keys equal to T: the first 192
// that arrive), the same id-order scan when more than 192 keys equal T (a marked id's value is looked up in the table there), the same counting placement.  Thread 0 then
// runs sample_rule over the <= 64 candidates in LDS and draws with word 0 of Philox4x32-10(seed, draws).  out[r]: pick, stuck flag, the word, n_cand, kept, the candidate
// ids (-1 behind n_cand) and probabilities (0 behind kept); the pick also goes into row_tok[tok_index] when that index is >= 0 (k_guide_rows' hand-over).  No id
// participates: pick = CONSTRAINT_EOS, stuck = 1, n_cand = kept = 0.  Table ids outside [0, n_vocab) are ignored; the ids of one table are distinct.  Logits are finite
// (-infinity through a bias is ordered like any value; NaN: unspecified).  The logits are read in place and never written; nothing beyond n_vocab floats of a row is read.
// No spinning, no flags between workgroups, no global atomics; every loop is bounded by n_vocab or by the table length.
// LDS: 12 KB static (8 KB histogram, 3 KB candidate lists, the ordered candidates) + dynamic 2 * constraint_words(n_vocab) bitmap words (8 KB at 32 001 ids).
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): 51 VGPRs, 89 SGPRs, no scratch, 12080 bytes of static LDS, occupancy 8 waves per SIMD.
// The extended rule (sample_chain) decides in k_sample_rows_ex: the same text up to the ordered candidates, then every thread enters sample_chain (its sequential sums are
// thread 0's, the order typical sampling needs is placed one lane per candidate); its scratch is the candidate lists' LDS, dead by then.  rows[r] carries the chain's
// parameters and the conversation's mu behind the plain descriptor, out[r] the mask of the candidates left in L, mu' and the observed surprise behind the plain result
// (stuck: mask 0, mu as a mirostat decision finds it, observed 0).  The contract above holds for it word for word.
// Resources of k_sample_rows_ex (gfx950, -Rpass-analysis=kernel-resource-usage): 54 VGPRs, 96 SGPRs, no scratch, 12096 bytes of static LDS, occupancy 8 waves per SIMD.
inline __device__ const SampleRow &smp_base(const SampleRow &r) { return r; }
inline __device__ const SampleRow &smp_base(const SampleRowEx &r) { return r.base; }
inline __device__ SampleOut &smp_base(SampleOut &o) { return o; }
inline __device__ SampleOut &smp_base(SampleOutEx &o) { return o.base; }
template <typename Row, typename Out>
__device__ __forceinline__ void sample_rows_body(const float *__restrict__ logits, int ld, int n_vocab, const Row *__restrict__ rows, const PenEntry *__restrict__ table,
                                                 Out *__restrict__ out_x, int *__restrict__ row_tok) {
    constexpr bool EX = std::is_same<Row, SampleRowEx>::value;
    constexpr int GT = SAMPLE_MAX, TIES = 256 - SAMPLE_MAX;
    extern __shared__ __attribute__((aligned(16))) unsigned smp_lds[];
    __shared__ unsigned hist[2048], sw[4], sres[2], ckey[256];
    __shared__ int cid[256], cnt[2], s_id[SAMPLE_MAX], s_res[2];
    __shared__ float cval[256], s_val[SAMPLE_MAX], s_p[SAMPLE_MAX];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const Row rx = rows[r];
    const SampleRow &sr = smp_base(rx);
    SampleOut &o = smp_base(out_x[r]);                                        // the plain result of row r
    if (tid < 2) cnt[tid] = 0;
    for (int i = tid; i < 2048; i += 256) hist[i] = 0;
    PickRow<true> row;                                                        // the transformed row's walk (pick_row.hpp); its barriers cover cnt and hist
    row.stage(logits, ld, n_vocab, sr.pen, table, sr.allowed, smp_lds, tid);
    auto each = [&](auto f) { row.each(tid, f); };
    // level 1, and the number of participating ids
    unsigned mine = 0;
    each([&](float v, int) { mine++; topn_hist_add(hist, true, topn_key(v) >> 21, lane); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += (unsigned)__shfl_xor((int)mine, o);
    if (lane == 0) sw[tid >> 6] = mine;
    __syncthreads();
    const unsigned total = sw[0] + sw[1] + sw[2] + sw[3];
    const uint32_t word = sample_word(sr.seed, sr.draws);
    __syncthreads();                                                          // sw is written again by topn_select
    if (total == 0) {                                                         // (uniform) nothing takes part: k_constrain_pick's answer
        if (tid < SAMPLE_MAX) { o.ids[tid] = -1; o.p[tid] = 0.0f; }
        if (tid == 0) {
            o.pick = CONSTRAINT_EOS; o.stuck = 1; o.word = word; o.n_cand = 0; o.kept = 0;
            if (row_tok && sr.tok_index >= 0) row_tok[sr.tok_index] = CONSTRAINT_EOS < n_vocab ? CONSTRAINT_EOS : 0;
            if constexpr (EX) {
                const ChainParams &cp = rx.chain;
                out_x[r].mask_lo = 0u; out_x[r].mask_hi = 0u; out_x[r].observed = 0.0f;
                out_x[r].mu = cp.mirostat == 2 && cp.mu != cp.mu ? smp::mul(2.0f, cp.tau) : cp.mu;
            }
        }
        return;
    }
    const int k = (int)min((unsigned)max(min(sr.top_k, SAMPLE_MAX), 1), total);
    unsigned b1, b2, b3, a1, a2, a3;
    topn_select(hist, 8, (unsigned)k, tid, sw, sres, b1, a1);
    for (int i = tid; i < 2048; i += 256) hist[i] = 0;
    __syncthreads();
    each([&](float v, int) { const unsigned key = topn_key(v); topn_hist_add(hist, (key >> 21) == b1, (key >> 10) & 2047u, lane); });
    __syncthreads();
    topn_select(hist, 8, (unsigned)k - a1, tid, sw, sres, b2, a2);
    const unsigned p2 = (b1 << 11) | b2;
    for (int i = tid; i < 1024; i += 256) hist[i] = 0;
    __syncthreads();
    each([&](float v, int) { const unsigned key = topn_key(v); topn_hist_add(hist, (key >> 10) == p2, key & 1023u, lane); });
    __syncthreads();
    topn_select(hist, 4, (unsigned)k - a1 - a2, tid, sw, sres, b3, a3);
    const unsigned T = (p2 << 10) | b3;
    const int n_gt = (int)(a1 + a2 + a3), need = k - n_gt;                    // n_gt < k keys lie above T, at least `need` >= 1 equal it
    // the collecting sweep
    each([&](float v, int i) {
        const unsigned key = topn_key(v);
        if (key > T) {
            const int p = atomicAdd(&cnt[0], 1);
            if (p < GT) { ckey[p] = key; cid[p] = i; cval[p] = v; }
        } else if (key == T) {
            const unsigned long long m = __ballot(1);
            const int leader = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&cnt[1], (int)__popcll(m));
            const int p = __shfl(base, leader) + (int)__popcll(m & ((1ull << lane) - 1ull));
            if (p < TIES) { ckey[GT + p] = key; cid[GT + p] = i; cval[GT + p] = v; }
        }
    });
    __syncthreads();
    int n_tie = cnt[1];
    if (n_tie > TIES) {   // (uniform) too many keys equal T to have been listed: the lowest `need` ids among them, 1024 ids per step, in id order
        int taken = 0;
        for (int base = 0; base < n_vocab && taken < need; base += 1024) {
            const int i0 = base + 4 * tid;
            unsigned m4 = 0; float v4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = i0 + j;
                if (i >= n_vocab || !row.is_allowed(i)) continue;
                const float v = row.value_of(i);                              // (a table id: its entry's value)
                if (topn_key(v) == T) { m4 |= 1u << j; v4[j] = v; }
            }
            const unsigned c = (unsigned)__popc(m4), inc = topn_wave_scan(c, lane);
            if (lane == 63) sw[tid >> 6] = inc;
            __syncthreads();
            int at = taken + (int)(inc - c);
            for (int w = 0; w < (tid >> 6); w++) at += (int)sw[w];
#pragma unroll
            for (int j = 0; j < 4; j++) if ((m4 >> j) & 1u) { if (at < need) { ckey[GT + at] = T; cid[GT + at] = i0 + j; cval[GT + at] = v4[j]; } at++; }
            taken += (int)(sw[0] + sw[1] + sw[2] + sw[3]);
            __syncthreads();
        }
        n_tie = need;
    }
    __syncthreads();
    // placement: a key above T goes behind the keys above it (equal ones by id); a key equal to T behind all of those and the lower ids of its own kind
    const bool is_gt = tid < n_gt, is_tie = tid >= GT && tid < GT + n_tie;
    if (is_gt || is_tie) {
        const unsigned mk = ckey[tid]; const int mi = cid[tid];
        int pos = is_gt ? 0 : n_gt;
        if (is_gt) { for (int c = 0; c < n_gt; c++) pos += (ckey[c] > mk || (ckey[c] == mk && cid[c] < mi)) ? 1 : 0; }
        else for (int c = GT; c < GT + n_tie; c++) pos += cid[c] < mi ? 1 : 0;
        if (pos < k) { s_id[pos] = mi; s_val[pos] = cval[tid]; }
    }
    __syncthreads();
    if constexpr (EX) {   // the candidate lists are dead: cval and cid become the chain's scratch (sa, sb | L, ord)
        __shared__ ChainRes s_chain;
        sample_chain(s_val, k, sr.temp, sr.top_p, rx.chain, word, tid, 256, s_p, cval, cval + SAMPLE_MAX, cid, cid + SAMPLE_MAX, &s_chain);
        if (tid == 0) {
            s_res[0] = s_id[s_chain.pick]; s_res[1] = s_chain.kept;
            out_x[r].mask_lo = s_chain.mask_lo; out_x[r].mask_hi = s_chain.mask_hi; out_x[r].mu = s_chain.mu; out_x[r].observed = s_chain.observed;
        }
    } else if (tid == 0) {
        int kept;
        const int j = sample_rule(s_val, k, sr.temp, sr.top_p, word, s_p, &kept);
        s_res[0] = s_id[j]; s_res[1] = kept;
    }
    __syncthreads();
    if (tid < SAMPLE_MAX) { o.ids[tid] = tid < k ? s_id[tid] : -1; o.p[tid] = tid < k ? s_p[tid] : 0.0f; }
    if (tid == 0) {
        const int id = s_res[0];
        o.pick = id; o.stuck = 0; o.word = word; o.n_cand = k; o.kept = s_res[1];
        if (row_tok && sr.tok_index >= 0) row_tok[sr.tok_index] = id;
    }
}
__global__ __launch_bounds__(256) void k_sample_rows(const float *__restrict__ logits, int ld, int n_vocab, const SampleRow *__restrict__ rows, const PenEntry *__restrict__ table,
                                                     SampleOut *__restrict__ out, int *__restrict__ row_tok) {
    sample_rows_body(logits, ld, n_vocab, rows, table, out, row_tok);
}
__global__ __launch_bounds__(256) void k_sample_rows_ex(const float *__restrict__ logits, int ld, int n_vocab, const SampleRowEx *__restrict__ rows, const PenEntry *__restrict__ table,
                                                        SampleOutEx *__restrict__ out, int *__restrict__ row_tok) {
    sample_rows_body(logits, ld, n_vocab, rows, table, out, row_tok);
}
bool launch_sample_rows_ex(const float *logits, int ld, int n_vocab, int n_rows, const SampleRowEx *rows, const PenEntry *table, SampleOutEx *out, int *row_tok, hipStream_t s) {
    const size_t lds = (size_t)2 * constraint_words(n_vocab) * 4;
    if (!logits || !rows || !out || n_rows < 1 || n_vocab < 1 || ld < n_vocab || lds + 12 * 1024 + 256 > 64 * 1024) { set_last_error("launch_sample_rows_ex: shape out of range"); return false; }
    note_kernel("k_sample_rows_ex");
    hipLaunchKernelGGL(k_sample_rows_ex, dim3((unsigned)n_rows), dim3(256), lds, s, logits, ld, n_vocab, rows, table, out, row_tok);
    return true;
}
bool launch_sample_rows(const float *logits, int ld, int n_vocab, int n_rows, const SampleRow *rows, const PenEntry *table, SampleOut *out, int *row_tok, hipStream_t s) {
    const size_t lds = (size_t)2 * constraint_words(n_vocab) * 4;
    if (!logits || !rows || !out || n_rows < 1 || n_vocab < 1 || ld < n_vocab || lds + 12 * 1024 + 256 > 64 * 1024) { set_last_error("launch_sample_rows: shape out of range"); return false; }
    note_kernel("k_sample_rows");
    hipLaunchKernelGGL(k_sample_rows, dim3((unsigned)n_rows), dim3(256), lds, s, logits, ld, n_vocab, rows, table, out, row_tok);
    return true;
}
// Verify pass epilogue under sampling (Engine::verify_draft_sampled), ONE workgroup of 1024, launched behind k_sample_rows over the pass's R rows: picks[r] is the decision of
// row r (x_{r + 1} of the rule in minigpt4_amd.h), tok[0 .. R) the pass's rows (tok[0] = x0, tok[1 ..] the draft).  m = the number of leading draft tokens the rows' own
// samples chose (tok[i + 1] == picks[i].pick for every i < m); row m becomes the conversation's state as k_draft_finish leaves it -- its logits row copied into the slot's
// row with the first argmax found in the same sweep (batch_finish_row<true>'s sweep: every thread visits its indices in ascending order, `>` keeps the first of equal values,
// -0.0 == +0.0; 16-byte loads when both strides allow them), greedy and feed token = that argmax, position p + 1 + m (n_past[slot] still holds p) -- and
// res = {m, picks [DRAFT_ROWS], stuck flags [DRAFT_ROWS]} (entries from R on are left alone).  The logits rows lie ld floats apart; nothing beyond n_vocab floats of a row is
// read.  No flags or counters between workgroups, no spinning, no atomics; every loop is bounded by n_vocab or by R.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): 17 VGPRs, 41 SGPRs, no scratch, 128 bytes of static LDS, occupancy 8 waves per SIMD.
// k_draft_sample_finish_ex: the same text over the extended decisions (k_sample_rows_ex's SampleOutEx blocks: the plain result leads each).
// Resources of k_draft_sample_finish_ex (gfx950, -Rpass-analysis=kernel-resource-usage): 17 VGPRs, 41 SGPRs, no scratch, 128 bytes of static LDS, as the plain instance.
inline __device__ const SampleOut &smp_base(const SampleOut &o) { return o; }
inline __device__ const SampleOut &smp_base(const SampleOutEx &o) { return o.base; }
template <typename Out>
__device__ __forceinline__ void draft_sample_finish_body(const float *__restrict__ logits, int ld, int n_vocab, int R, const int *__restrict__ tok, const Out *__restrict__ picks,
                                                         const int *__restrict__ row_slot, int *__restrict__ n_past, int *__restrict__ argmax, int *__restrict__ feed,
                                                         float *__restrict__ slot_logits, int *__restrict__ res) {
    int m = 0;
    while (m < R - 1 && tok[m + 1] == smp_base(picks[m]).pick) m++;       // every thread: R <= 8 words, all in cache
    const int slot = row_slot[0];
    const float *x = logits + (size_t)m * ld;
    float *keep = slot_logits + (size_t)slot * n_vocab;
    float best = -INFINITY; int bi = 0x7FFFFFFF;
    const int n4 = ((n_vocab | ld) & 3) == 0 ? n_vocab >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += 1024) {
        const float4 v = reinterpret_cast<const float4 *>(x)[i]; reinterpret_cast<float4 *>(keep)[i] = v;
        if (v.x > best) { best = v.x; bi = 4 * i; } if (v.y > best) { best = v.y; bi = 4 * i + 1; } if (v.z > best) { best = v.z; bi = 4 * i + 2; } if (v.w > best) { best = v.w; bi = 4 * i + 3; }
    }
    for (int i = 4 * n4 + threadIdx.x; i < n_vocab; i += 1024) { const float v = x[i]; keep[i] = v; if (v > best) { best = v; bi = i; } }
    __shared__ float sv[16]; __shared__ int si[16];
    argmax_wave(best, bi);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x < R) { res[1 + threadIdx.x] = smp_base(picks[threadIdx.x]).pick; res[1 + DRAFT_ROWS + threadIdx.x] = smp_base(picks[threadIdx.x]).stuck; }
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++) argmax_combine(best, bi, sv[w], si[w]);
        const int id = bi == 0x7FFFFFFF ? 0 : bi;
        argmax[slot] = id; feed[slot] = id; n_past[slot] += 1 + m; res[0] = m;
    }
}
__global__ __launch_bounds__(1024) void k_draft_sample_finish(const float *__restrict__ logits, int ld, int n_vocab, int R, const int *__restrict__ tok, const SampleOut *__restrict__ picks,
                                                             const int *__restrict__ row_slot, int *__restrict__ n_past, int *__restrict__ argmax, int *__restrict__ feed,
                                                             float *__restrict__ slot_logits, int *__restrict__ res) {
    draft_sample_finish_body(logits, ld, n_vocab, R, tok, picks, row_slot, n_past, argmax, feed, slot_logits, res);
}
__global__ __launch_bounds__(1024) void k_draft_sample_finish_ex(const float *__restrict__ logits, int ld, int n_vocab, int R, const int *__restrict__ tok, const SampleOutEx *__restrict__ picks,
                                                                const int *__restrict__ row_slot, int *__restrict__ n_past, int *__restrict__ argmax, int *__restrict__ feed,
                                                                float *__restrict__ slot_logits, int *__restrict__ res) {
    draft_sample_finish_body(logits, ld, n_vocab, R, tok, picks, row_slot, n_past, argmax, feed, slot_logits, res);
}
bool launch_draft_sample_finish(const float *logits, int ld, int n_vocab, int R, const int *tok, const SampleOutEx *picks, const int *row_slot, int *n_past, int *argmax, int *feed,
                                float *slot_logits, int *res, hipStream_t s) {
    if (!logits || !tok || !picks || !row_slot || !n_past || !argmax || !feed || !slot_logits || !res || R < 1 || R > DRAFT_ROWS || n_vocab < 1 || ld < n_vocab) {
        set_last_error("launch_draft_sample_finish: shape out of range"); return false;
    }
    note_kernel("k_draft_sample_finish_ex");
    hipLaunchKernelGGL(k_draft_sample_finish_ex, dim3(1), dim3(1024), 0, s, logits, ld, n_vocab, R, tok, picks, row_slot, n_past, argmax, feed, slot_logits, res);
    return true;
}
bool launch_draft_sample_finish(const float *logits, int ld, int n_vocab, int R, const int *tok, const SampleOut *picks, const int *row_slot, int *n_past, int *argmax, int *feed,
                                float *slot_logits, int *res, hipStream_t s) {
    if (!logits || !tok || !picks || !row_slot || !n_past || !argmax || !feed || !slot_logits || !res || R < 1 || R > DRAFT_ROWS || n_vocab < 1 || ld < n_vocab) {
        set_last_error("launch_draft_sample_finish: shape out of range"); return false;
    }
    note_kernel("k_draft_sample_finish");
    hipLaunchKernelGGL(k_draft_sample_finish, dim3(1), dim3(1024), 0, s, logits, ld, n_vocab, R, tok, picks, row_slot, n_past, argmax, feed, slot_logits, res);
    return true;
}
// batched decode prologue: the host's view of each row's position (a conversation may have been reset) -> n_past[slot]
__global__ void k_batch_begin(int *__restrict__ n_past, const int *__restrict__ row_slot, const int *__restrict__ row_pos, int B) {
    const int r = threadIdx.x;
    if (r < B) n_past[row_slot[r]] = row_pos[r];
}
void launch_batch_begin(int *n_past, const int *row_slot, const int *row_pos, int B, hipStream_t s) { hipLaunchKernelGGL(k_batch_begin, dim3(1), dim3(64), 0, s, n_past, row_slot, row_pos, B); }
// end of a decode step: the KV position advances and the greedy token becomes the next input (the host may overwrite it)
__global__ void k_advance(int *n_past, int n, int *tok0, const int *argmax) {
    if (MV_PIN_AT_ENTRY) asm volatile("" ::"s"(n_past), "s"(n), "s"(tok0), "s"(argmax));
    *n_past += n; if (tok0) *tok0 = *argmax;
}
void launch_advance(int *n_past, int n, int *tok0, const int *argmax, hipStream_t s) { note_kernel("k_advance"); hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, n_past, n, tok0, argmax); }
// Profiling gate (Engine::profile_sites): one wave that keeps the stream busy for `us` microseconds (s_memrealtime: the constant 100 MHz clock) while the host
// queues the step's launches behind it, so the per-site event pairs time the GPU and not the host's launch rate.  Bounded: at most 2^20 polls even if the clock stood still.
__global__ void k_delay(int us) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime(), ticks = (unsigned long long)us * 100ull;
    for (int i = 0; i < (1 << 20) && __builtin_amdgcn_s_memrealtime() - t0 < ticks; i++) __builtin_amdgcn_s_sleep(32);
}
void launch_delay(int us, hipStream_t s) { hipLaunchKernelGGL(k_delay, dim3(1), dim3(1), 0, s, us); }

}  // namespace mg4
