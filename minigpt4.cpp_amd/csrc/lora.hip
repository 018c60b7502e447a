// Run-time LoRA adapters: y = W x + s * B (A x), one adapter per CONVERSATION, rows of different adapters (and of none) in the same weight pass.
// The base mat-vec / mat-mul launches are untouched, whatever their weight type; the two kernels here add the low-rank term to the outputs those launches wrote:
//   k_lora_down   t[ks][row][j] = sum over K slab ks of A[j][k] * f(x[row])[k]      f: plain | x * g (RMS norm, unnormalised) | silu(h1) * h3
//   k_lora_up     y[m][row][n] += s * sum_j B_m[n][j] * (rs * sum_ks t[ks][row][off_m + j])
// A is the row-concatenated image of the targets that share the input (q | k | v, w1 | w3): one down launch serves them, one up launch covers up to three targets.
// The RMS factor is a row-wide scalar, so the down kernel streams A . (x * g) at once and leaves its slab's partial sum of x^2 next to t; the up kernel forms
// rs = 1 / sqrt(mean + eps) from the slabs' sums in slab order.  Nothing crosses workgroups but through t: no atomics, the same inputs give the same bits.
// Every kernel finds its rows' adapters in device memory (adapter[slot] / scale[slot], slot from the row like the positions from n_past), so a captured decode graph
// survives a change of assignment; index -1 = the workgroup (vector forms: one row) returns at once.
// Two forms of each, chosen by row count (lora_form_for):
//   vector  x stays fp32 exactly, fp16 weights read with 16-byte loads, fp32 accumulation.  Down: one workgroup per (K slab, row, 64 rows of A), its f(x) slab in LDS,
//           one wave per A row.  Up: one thread per output column reading that column's <= 128 contiguous bytes of B.
//   MFMA    32-row tiles on v_mfma_f32_32x32x16_f16, grid.y over the loaded adapters: a workgroup reads its tile's adapter indices first, returns when none of its rows
//           uses its adapter and stores only the rows that do.  Down converts f(x) to fp16 into LDS once per K step of 64 and streams A from memory into the B operand;
//           up holds the fp16 t tile in LDS and streams B over 32-column tiles, one per wave.
// Choices that are NOT measured yet (no timing of these kernels exists): the switch-over at more than 8 rows (the verify pass's 8 rows stay on the vector form), K slabs of
// 512 (vector) / 2048 (MFMA) elements.
#include <algorithm>

#include "kernels.hpp"

namespace mg4 {

namespace {
typedef _Float16 lh8_t __attribute__((ext_vector_type(8)));
typedef float lf16_t __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int lora_slot(const LoraRows &R, int row) { return R.row_slot ? R.row_slot[(size_t)row * R.stride] : R.slot0; }
__device__ __forceinline__ int lora_adapter(const LoraRows &R, int row) { return R.adapter[lora_slot(R, row)]; }
// f(x) of one element; sq += x^2 for the RMS mode
__device__ __forceinline__ float lora_f(int mode, float x, float y, float &sq) {
    if (mode == LORA_RMS) { sq += x * x; return x * y; }
    if (mode == LORA_SILU) return (x / (1.0f + expf(-x))) * y;
    return x;
}
__device__ __forceinline__ float lora_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// rs of a row: 1 / sqrt(mean(x^2) + eps) from the slabs' partial sums in slab order (row_prep.hpp's row_scale)
__device__ __forceinline__ float lora_rs(int mode, const float *ssq, int ks_n, int N, int row, int n_in) {
    if (mode != LORA_RMS) return 1.0f;
    float tot = 0.0f;
    for (int ks = 0; ks < ks_n; ks++) tot += ssq[(size_t)ks * N + row];
    return 1.0f / sqrtf(tot / (float)n_in + 1e-6f);
}

constexpr int VSLAB = LORA_SLAB_VEC;

// grid (ks, row, 64-row group of A), 256 threads
__global__ __launch_bounds__(256) void k_lora_down(const LoraGroup G, const LoraRows R, int N, int n_in, int mode, const float *x, const float *y2, float *t, float *ssq) {
    const int ks = blockIdx.x, row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = lora_adapter(R, row);
    if (a < 0) return;
    const __half *A = G.A[a];
    const int rcat = G.rcat[a], j0 = blockIdx.z * 64;
    if (!A || j0 >= rcat) return;
    __shared__ float xs[VSLAB];
    __shared__ float red[4];
    const int k0 = ks * VSLAB, len = min(n_in - k0, VSLAB);
    const float *xr = x + (size_t)row * n_in + k0;
    const float *yr = mode == LORA_PLAIN ? xr : mode == LORA_RMS ? y2 + k0 : y2 + (size_t)row * n_in + k0;
    float sq = 0.0f;
    for (int i = tid; i < len; i += 256) xs[i] = lora_f(mode, xr[i], yr[i], sq);
    if (mode == LORA_RMS && blockIdx.z == 0) { sq = lora_wave_sum(sq); if (lane == 0) red[wave] = sq; }
    __syncthreads();
    if (mode == LORA_RMS && blockIdx.z == 0 && tid == 0) ssq[(size_t)ks * N + row] = ((red[0] + red[1]) + red[2]) + red[3];
    const int j1 = min(rcat, j0 + 64);
    for (int j = j0 + wave; j < j1; j += 4) {
        const __half *ar = A + (size_t)j * n_in + k0;
        float acc = 0.0f;
        for (int c = lane * 8; c < len; c += 512) {
            const uint4 w = *reinterpret_cast<const uint4 *>(ar + c);
            const __half2 *h = reinterpret_cast<const __half2 *>(&w);
#pragma unroll
            for (int i = 0; i < 4; i++) { const float2 f = __half22float2(h[i]); acc = fmaf(f.x, xs[c + 2 * i], acc); acc = fmaf(f.y, xs[c + 2 * i + 1], acc); }
        }
        acc = lora_wave_sum(acc);
        if (lane == 0) t[((size_t)ks * N + row) * LORA_TCAT + j] = acc;
    }
}

// grid (ceil(n_out / 256), row, target), 256 threads
__global__ __launch_bounds__(256) void k_lora_up(const LoraGroup G, const LoraRows R, const LoraOut Y, int N, int n_in, int mode, int n_out, int ldy, int ks_n, const float *t,
                                                 const float *ssq) {
    const int row = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
    float *y = Y.y[m];
    if (!y) return;
    const int slot = lora_slot(R, row), a = R.adapter[slot];
    if (a < 0) return;
    const __half *B = G.B[a][m];
    if (!B) return;
    const int rp = G.rp[a], off = G.aoff[a][m];
    __shared__ float ts[LORA_RANK_MAX];
    if (tid < rp) {
        float v = 0.0f;
        for (int ks = 0; ks < ks_n; ks++) v += t[((size_t)ks * N + row) * LORA_TCAT + off + tid];
        ts[tid] = v * lora_rs(mode, ssq, ks_n, N, row, n_in);
    }
    __syncthreads();
    const int n = blockIdx.x * 256 + tid;
    if (n >= n_out) return;
    const __half *br = B + (size_t)n * rp;
    float acc = 0.0f;
    for (int j = 0; j < rp; j += 8) {
        const uint4 w = *reinterpret_cast<const uint4 *>(br + j);
        const __half2 *h = reinterpret_cast<const __half2 *>(&w);
#pragma unroll
        for (int i = 0; i < 4; i++) { const float2 f = __half22float2(h[i]); acc = fmaf(f.x, ts[j + 2 * i], acc); acc = fmaf(f.y, ts[j + 2 * i + 1], acc); }
    }
    y[(size_t)row * ldy + n] += (G.alpha_r[a] * R.scale[slot]) * acc;
}

constexpr int MROWS = 32, MKSTEP = 64, MLD = MKSTEP + 8;   // LDS row stride 144 bytes: 16-byte aligned chunks, rows on different banks

// the tile's adapter indices -> sa[]; false: no row of the tile uses adapter a
__device__ __forceinline__ bool lora_tile_rows(const LoraRows &R, int r0, int N, int a, int *sa) {
    if (threadIdx.x < MROWS) { const int row = r0 + threadIdx.x; sa[threadIdx.x] = row < N ? lora_adapter(R, row) : -1; }
    __syncthreads();
    bool any = false;
    for (int i = 0; i < MROWS; i++) any = any || sa[i] == a;
    return any;
}

// grid (row tile, adapter, ks), 256 threads: wave w owns the 32-column tiles w and w + 4 of t (rcat <= 192: six tiles)
__global__ __launch_bounds__(256) void k_lora_down_mfma(const LoraGroup G, const LoraRows R, int N, int n_in, int mode, int slab, const float *x, const float *y2, float *t, float *ssq) {
    const int r0 = blockIdx.x * MROWS, a = blockIdx.y, ks = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, hh = lane >> 5;
    const __half *A = G.A[a];
    if (!A) return;
    __shared__ int sa[MROWS];
    __shared__ __align__(16) __half xs[MROWS * MLD];
    if (!lora_tile_rows(R, r0, N, a, sa)) return;
    const int rcat = G.rcat[a], k0 = ks * slab, k1 = min(n_in, k0 + slab);
    lf16_t acc[2];
#pragma unroll
    for (int i = 0; i < 16; i++) { acc[0][i] = 0.0f; acc[1][i] = 0.0f; }
    const int crow = tid >> 3, cc = (tid & 7) * 8, grow = r0 + crow;     // this thread's 8 elements of the converted tile
    float sq = 0.0f;
    for (int kk = k0; kk < k1; kk += MKSTEP) {
        // this K step's pieces of A, requested ahead of the conversion: they do not depend on LDS
        lh8_t bf[2][4];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int col = (wave + 4 * u) * 32 + lrow;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = kk + q * 16 + hh * 8;
                uint4 w = make_uint4(0u, 0u, 0u, 0u);
                if (col < rcat && k < k1) w = *reinterpret_cast<const uint4 *>(A + (size_t)col * n_in + k);
                bf[u][q] = __builtin_bit_cast(lh8_t, w);
            }
        }
        lh8_t hv;
#pragma unroll
        for (int i = 0; i < 8; i++) hv[i] = (_Float16)0.0f;
        if (grow < N && kk + cc < k1) {
            const float *xr = x + (size_t)grow * n_in + kk + cc;
            const float *yr = mode == LORA_PLAIN ? xr : mode == LORA_RMS ? y2 + kk + cc : y2 + (size_t)grow * n_in + kk + cc;
            const float4 xa = *reinterpret_cast<const float4 *>(xr), xb = *reinterpret_cast<const float4 *>(xr + 4);
            const float4 ya = *reinterpret_cast<const float4 *>(yr), yb = *reinterpret_cast<const float4 *>(yr + 4);
            const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w}, yv[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
#pragma unroll
            for (int i = 0; i < 8; i++) hv[i] = (_Float16)lora_f(mode, xv[i], yv[i], sq);
        }
        *reinterpret_cast<lh8_t *>(&xs[crow * MLD + cc]) = hv;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const lh8_t af = *reinterpret_cast<const lh8_t *>(&xs[lrow * MLD + q * 16 + hh * 8]);
#pragma unroll
            for (int u = 0; u < 2; u++) if ((wave + 4 * u) * 32 < rcat) acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf[u][q], acc[u], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int col = (wave + 4 * u) * 32 + lrow;
        if (col >= rcat) continue;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int lr = (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (sa[lr] == a) t[((size_t)ks * N + r0 + lr) * LORA_TCAT + col] = acc[u][r];
        }
    }
    if (mode == LORA_RMS) {   // the eight threads of a tile row sit in adjacent lanes
        sq += __shfl_xor(sq, 1, 64); sq += __shfl_xor(sq, 2, 64); sq += __shfl_xor(sq, 4, 64);
        if ((tid & 7) == 0 && sa[crow] == a) ssq[(size_t)ks * N + grow] = sq;
    }
}

// grid (ceil(n_out / 128), adapter, row tile * 3 + target), 256 threads: one 32-column tile per wave
__global__ __launch_bounds__(256) void k_lora_up_mfma(const LoraGroup G, const LoraRows R, const LoraOut Y, int N, int n_in, int mode, int n_out, int ldy, int ks_n, const float *t,
                                                      const float *ssq) {
    const int a = blockIdx.y, m = blockIdx.z % LORA_TARGETS, r0 = (blockIdx.z / LORA_TARGETS) * MROWS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, hh = lane >> 5;
    float *y = Y.y[m];
    const __half *B = G.B[a][m];
    if (!y || !B) return;
    __shared__ int sa[MROWS];
    __shared__ float sfac[MROWS];
    __shared__ __align__(16) __half ts[MROWS * MLD];
    if (!lora_tile_rows(R, r0, N, a, sa)) return;
    const int rp = G.rp[a], off = G.aoff[a][m];
    {   // t tile: slabs summed in slab order, times the row's RMS factor, rounded to fp16; rows of other adapters and the padding are zero
        const int crow = tid >> 3, cc = (tid & 7) * 8, grow = r0 + crow;
        const bool mine = sa[crow] == a;
        const float rs = mine ? lora_rs(mode, ssq, ks_n, N, grow, n_in) : 0.0f;
        lh8_t hv;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            float v = 0.0f;
            if (mine && cc + i < rp) for (int ks = 0; ks < ks_n; ks++) v += t[((size_t)ks * N + grow) * LORA_TCAT + off + cc + i];
            hv[i] = (_Float16)(v * rs);
        }
        *reinterpret_cast<lh8_t *>(&ts[crow * MLD + cc]) = hv;
        if ((tid & 7) == 0) sfac[crow] = mine ? G.alpha_r[a] * R.scale[lora_slot(R, grow)] : 0.0f;
    }
    __syncthreads();
    const int col = blockIdx.x * 128 + wave * 32 + lrow;
    lf16_t acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;
    for (int q = 0; q < rp / 16; q++) {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (col < n_out) w = *reinterpret_cast<const uint4 *>(B + (size_t)col * rp + q * 16 + hh * 8);
        const lh8_t af = *reinterpret_cast<const lh8_t *>(&ts[lrow * MLD + q * 16 + hh * 8]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, __builtin_bit_cast(lh8_t, w), acc, 0, 0, 0);
    }
    if (col >= n_out) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int lr = (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (sa[lr] == a) y[(size_t)(r0 + lr) * ldy + col] += sfac[lr] * acc[r];
    }
}
}  // namespace

int lora_form_for(const LaunchTuning &tune, int N) { return tune.lora_form == 1 || tune.lora_form == 2 ? tune.lora_form : N > 8 ? 2 : 1; }
int lora_ks(int n_in, int form) {
    if (form == 1) return (n_in + LORA_SLAB_VEC - 1) / LORA_SLAB_VEC;
    return (n_in + LORA_SLAB_MFMA - 1) / LORA_SLAB_MFMA;
}
size_t lora_ws_floats(int N, int n_in) { return (size_t)lora_ks(n_in, 1) * (size_t)N * (LORA_TCAT + 1); }

static void lora_check(int n_adapters, int N, int n_in, int mode) {
    if (n_adapters < 1 || n_adapters > LORA_MAX || N < 1 || n_in < 8 || n_in % 8 || mode < LORA_PLAIN || mode > LORA_SILU)
        throw HipError{hipErrorInvalidValue, "lora launch: adapters outside 1..8, no rows, n_in not a multiple of 8 or an unknown mode", __FILE__, __LINE__};
}
int launch_lora_down(const LoraGroup &G, int n_adapters, const LoraRows &R, int N, int n_in, int mode, const float *x, const float *y2, float *t, float *ssq, const LaunchTuning &tune,
                     hipStream_t s) {
    lora_check(n_adapters, N, n_in, mode);
    const int form = lora_form_for(tune, N), ks = lora_ks(n_in, form);
    int rcat = 0;
    for (int a = 0; a < n_adapters; a++) if (G.A[a]) rcat = std::max(rcat, G.rcat[a]);
    if (rcat < 1 || rcat > LORA_TCAT) throw HipError{hipErrorInvalidValue, "lora down: no adapter has rows here, or more than 192", __FILE__, __LINE__};
    if (form == 1) hipLaunchKernelGGL(k_lora_down, dim3(ks, N, (rcat + 63) / 64), dim3(256), 0, s, G, R, N, n_in, mode, x, y2, t, ssq);
    else hipLaunchKernelGGL(k_lora_down_mfma, dim3((N + MROWS - 1) / MROWS, n_adapters, ks), dim3(256), 0, s, G, R, N, n_in, mode, LORA_SLAB_MFMA, x, y2, t, ssq);
    return ks;
}
void launch_lora_up(const LoraGroup &G, int n_adapters, const LoraRows &R, const LoraOut &Y, int N, int n_in, int mode, int n_out, int ldy, int ks, const float *t, const float *ssq,
                    const LaunchTuning &tune, hipStream_t s) {
    lora_check(n_adapters, N, n_in, mode);
    if (n_out < 1 || ldy < n_out || ks < 1) throw HipError{hipErrorInvalidValue, "lora up: bad output shape", __FILE__, __LINE__};
    if (lora_form_for(tune, N) == 1) hipLaunchKernelGGL(k_lora_up, dim3((n_out + 255) / 256, N, LORA_TARGETS), dim3(256), 0, s, G, R, Y, N, n_in, mode, n_out, ldy, ks, t, ssq);
    else hipLaunchKernelGGL(k_lora_up_mfma, dim3((n_out + 127) / 128, n_adapters, ((N + MROWS - 1) / MROWS) * LORA_TARGETS), dim3(256), 0, s, G, R, Y, N, n_in, mode, n_out, ldy, ks, t, ssq);
}

}  // namespace mg4
