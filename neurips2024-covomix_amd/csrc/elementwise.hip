// Memory-bound kernels of the CoVoMix vector field + library-wide error plumbing (gfx950).
//   cvx_adarmsnorm_f32          AdaptiveRMSNorm / RMSNorm       (acoustic.py:165-204)
//   cvx_dwconv31_gelu_res_f32   ConvPositionEmbed + residual    (acoustic.py:141-161, :508)
//   cvx_cfg_combine_axpy_f32    CFG combine + ODE stage update  (acoustic.py:428; torchdiffeq midpoint)
//   cvx_rk_stage_f32            CFG combine + one explicit Runge-Kutta stage, per-row guidance scale
//   cvx_rk_stage_err_f32        the last stage of a step + the embedded error estimate's sums per chunk of a sequence
//   cvx_rk_err_finish_f32       chunk sums -> one (sum delta^2, sum o^2) per (step, sequence)
//   cvx_embed_gather_f32        step-invariant to_embed columns (acoustic.py:473-503)
//   cvx_time_fourier_f32        LearnedSinusoidalPosEmb         (acoustic.py:107-111)
//   cvx_wav_to_int16            mel_decode_to_wav tail          (monologue_generation.py:55-57)
// All are HBM-bound: 16-byte coalesced accesses over the channel axis, wavefront (64-lane)
// shuffles for the row reduction, no LDS needed.
#include "cvx_common.h"
#include <algorithm>
#include <stdarg.h>
#include <string.h>

// ---------------------------------------------------------------- error string
static thread_local char g_err[512] = "";
void cvx_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* cvx_last_error_string(void) { return g_err; }

#include <mutex>
#include <map>
#include <set>
#include <utility>
void cvx_allow_dynamic_lds(const void* kernel, int bytes)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, int> granted;       // largest size asked for so far, per (device, kernel)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    int& g = granted[std::make_pair(dev, kernel)];
    if (bytes > g) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        g = bytes;
    }
}
int cvx_device_cus()
{
    static std::mutex mu;
    static int n_cu[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    if (n_cu[dev] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        n_cu[dev] = v;
    }
    return n_cu[dev];
}
extern "C" int cvx_stream_create_cu_mask(const uint32_t* mask, int32_t n_words, void** out)
{
    CVX_REQUIRE(mask && out && n_words > 0 && n_words <= 64, "stream_create_cu_mask: bad arguments");
    int bits = 0;
    for (int i = 0; i < n_words; ++i) bits += __builtin_popcount(mask[i]);
    CVX_REQUIRE(bits > 0, "stream_create_cu_mask: empty mask");
    hipStream_t st = nullptr;
    const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)n_words, mask);
    if (e != hipSuccess) { cvx_set_error("stream_create_cu_mask: hipExtStreamCreateWithCUMask failed: %s", hipGetErrorString(e)); return CVX_EHIP; }
    *out = reinterpret_cast<void*>(st);
    return CVX_OK;
}
extern "C" int cvx_stream_destroy(void* stream)
{
    CVX_REQUIRE(stream, "stream_destroy: the NULL stream");
    const hipError_t e = hipStreamDestroy(reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) { cvx_set_error("stream_destroy: %s", hipGetErrorString(e)); return CVX_EHIP; }
    return CVX_OK;
}
extern "C" int cvx_saturation_flag_reset(cvx_stream_t s)
{
    uint32_t* f = cvx_sat_flag_for(s);
    CVX_REQUIRE(f && (reinterpret_cast<uintptr_t>(f) & 3) == 0, "saturation_flag_reset: the context carries no (4-byte aligned) saturation flag");
    if (hipMemsetAsync(f, 0, sizeof(uint32_t), cvx_hip_stream(s)) != hipSuccess) { cvx_set_error("saturation_flag: memset failed"); return CVX_EHIP; }
    return CVX_OK;
}
extern "C" int cvx_saturation_flag_query(uint32_t* host_out, int32_t reset, cvx_stream_t s)
{
    uint32_t* f = cvx_sat_flag_for(s);
    CVX_REQUIRE(f && host_out, "saturation_flag_query: the context carries no saturation flag / null output");
    hipStream_t st = cvx_hip_stream(s);
    if (hipMemcpyAsync(host_out, f, sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { cvx_set_error("saturation_flag: read failed: %s", hipGetErrorString(hipGetLastError())); return CVX_EHIP; }
    if (reset && hipMemsetAsync(f, 0, sizeof(uint32_t), st) != hipSuccess) { cvx_set_error("saturation_flag: memset failed"); return CVX_EHIP; }
    return CVX_OK;
}
// Clock stamps (bench.py): {shader-clock cycle counter, 100 MHz real-time counter} PER COMPUTE UNIT: the cycle counter belongs to the CU
// (stamps of two CUs of one XCD differ by arbitrary offsets - a per-XCD slot gave negative clocks over short regions), so a slot is
// (XCD, the CU / shader-array / shader-engine bits of HW_ID) and the caller pairs the two stamps of the SAME slot.  Two calls around a
// busy region give the shader clock it ran at, per CU; the hwmon file shows one XCD's momentary value, and config 2's time differs
// between boxes that report the same one.  4096 short blocks: the dispatcher spreads them over (nearly) every CU.
namespace {
__global__ __launch_bounds__(64) void clock_stamp_kernel(unsigned long long* __restrict__ out)
{
    unsigned xcc, hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    __builtin_amdgcn_s_sleep(64);                                        // (keeps the block resident long enough for the others to land elsewhere)
    const unsigned long long t = __builtin_readcyclecounter(), r = __builtin_amdgcn_s_memrealtime();
    const unsigned slot = ((xcc & 7) << 8) | ((hwid >> 8) & 0xFF);      // HW_ID[15:8] = CU_ID, SH_ID, SE_ID
    if (threadIdx.x == 0) { out[2 * slot] = t; out[2 * slot + 1] = r; }
}
}
extern "C" int cvx_clock_stamps(uint64_t* stamps_dev, cvx_stream_t s)
{
    CVX_REQUIRE(stamps_dev && (reinterpret_cast<uintptr_t>(stamps_dev) & 7) == 0, "clock_stamps: null / unaligned output");
    hipLaunchKernelGGL(clock_stamp_kernel, dim3(4096), dim3(64), 0, cvx_hip_stream(s), reinterpret_cast<unsigned long long*>(stamps_dev));
    CVX_CHECK_LAUNCH("cvx_clock_stamps");
    return CVX_OK;
}
extern "C" int cvx_version(void) { return CVX_ABI_VERSION; }

namespace {

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
// split 4 floats into fp16 (hi, lo) and store 8 bytes each (for GEMMs that take their A operand pre-split)
__device__ __forceinline__ void store_split4(_Float16* hi, _Float16* lo, int64_t off, const f32x4 o, CvxSat& amax)
{
    cvx_amax4(amax, o);
    // lo == hi + 32: INTERLEAVED pair, [hi 32 | lo 32] per block of 32 values (one 128-byte line per K-step and row for
    // the consumer GEMM's DMA); the mapping is a function of the flat offset because every row is a multiple of 32 wide
    if (lo == hi + 32) off = ((off >> 5) << 6) | (off & 31);
    f16x4_t h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x = fminf(fmaxf(o[e], -65504.f), 65504.f);
        h[e] = (_Float16)x;
        l[e] = (_Float16)(x - (float)h[e]);
    }
    *reinterpret_cast<f16x4_t*>(hi + off) = h;
    if (lo) *reinterpret_cast<f16x4_t*>(lo + off) = l;      // lo == NULL: hi halves only
}

// ---------------------------------------------------------------- AdaRMSNorm
// one wavefront per row; the row stays in registers when D <= 256*NV.
template <int NV>
__global__ __launch_bounds__(256) void adarmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y,
                                                        _Float16* __restrict__ y_hi, _Float16* __restrict__ y_lo,
                                                        int64_t rows, int D, int64_t rows_per_group, float scale, float eps,
                                                        const float* __restrict__ split_scale, uint32_t* __restrict__ sat)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    CvxSat amax;
    const float ssc = split_scale ? *split_scale : 1.f;      // power-of-two pre-scale of the split copy (device scalar)
    const float* xr = x + row * D;
    const int64_t g = row / rows_per_group;
    const float* gr = gamma + g * D;
    const float* br = beta ? beta + g * D : nullptr;
    float* yr = y ? y + row * D : nullptr;
    const int nvec = D >> 2;

    // every load of the row's pass is requested up front - x, and the item's gamma / beta rows (L2 hits) that used to be
    // requested only behind the wave reduction, one exposed round trip per row later
    f32x4 v[NV], gv[NV], bv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = lane + 64 * i;
        if (j < nvec) v[i] = gload4(xr + 4 * j);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = lane + 64 * i;
        if (j < nvec) {
            gv[i] = gload4(gr + 4 * j);
            if (br) bv[i] = gload4(br + 4 * j);
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = lane + 64 * i;
        if (j < nvec) ss += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
    }
    ss = wave_sum(ss);
    const float inv = scale / fmaxf(sqrtf(ss), eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = lane + 64 * i;
        if (j < nvec) {
            const f32x4 gg = gv[i];
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = v[i][e] * inv * gg[e];
            if (br) {
                const f32x4 bb = bv[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += bb[e];
            }
            if (y) *reinterpret_cast<f32x4*>(yr + 4 * j) = o;
            if (y_hi) { const f32x4 os = {o[0] * ssc, o[1] * ssc, o[2] * ssc, o[3] * ssc}; store_split4(y_hi, y_lo, row * D + 4 * j, os, amax); }
        }
    }
    cvx_sat_commit(sat, amax);
}

// generic-D fallback: two passes over the row (second pass hits L1/L2)
__global__ __launch_bounds__(256) void adarmsnorm_generic_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ y,
                                                                _Float16* __restrict__ y_hi, _Float16* __restrict__ y_lo,
                                                                int64_t rows, int D, int64_t rows_per_group, float scale, float eps,
                                                                const float* __restrict__ split_scale, uint32_t* __restrict__ sat)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    CvxSat amax;
    const float ssc = split_scale ? *split_scale : 1.f;
    const float* xr = x + row * D;
    const int64_t g = row / rows_per_group;
    float ss = 0.f;
    for (int j = lane; j < (D >> 2); j += 64) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xr + 4 * j);
        ss += t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3];
    }
    ss = wave_sum(ss);
    const float inv = scale / fmaxf(sqrtf(ss), eps);
    for (int j = lane; j < (D >> 2); j += 64) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xr + 4 * j);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(gamma + g * D + 4 * j);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = t[e] * inv * gg[e];
        if (beta) {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(beta + g * D + 4 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += bb[e];
        }
        if (y) *reinterpret_cast<f32x4*>(y + row * D + 4 * j) = o;
        if (y_hi) { const f32x4 os = {o[0] * ssc, o[1] * ssc, o[2] * ssc, o[3] * ssc}; store_split4(y_hi, y_lo, row * D + 4 * j, os, amax); }
    }
    cvx_sat_commit(sat, amax);
}

// ---------------------------------------------------------------- depthwise conv k=31 + GELU + residual
// channels-last [Bt,T,C]: a thread owns one channel and TT consecutive frames; every global
// access is a 256-byte coalesced row segment across the block's 64 channels x 4... (one wave = 64 channels).
constexpr int DW_K = 31, DW_TT = 16;
__global__ __launch_bounds__(256) void dwconv31_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ y,
                                                      int T, int C, const int* __restrict__ cu_seqlens)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int t0 = blockIdx.y * DW_TT;
    int64_t base = (int64_t)blockIdx.z * T * C;
    if (cu_seqlens) {                 // ragged batch: sequence z = rows [cu[z], cu[z+1]) of the packed tensor, zero-padded at ITS ends
        const int r0 = cu_seqlens[blockIdx.z];
        T = cu_seqlens[blockIdx.z + 1] - r0;
        base = (int64_t)r0 * C;
        if (t0 >= T) return;          // block-uniform: the grid is sized for the longest sequence
    }
    float wk[DW_K];
#pragma unroll
    for (int k = 0; k < DW_K; ++k) wk[k] = w[c * DW_K + k];
    // window of DW_TT + 30 frames held in registers; every index below is a compile-time constant
    float xs[DW_TT + DW_K - 1];
#pragma unroll
    for (int i = 0; i < DW_TT + DW_K - 1; ++i) {
        const int t = t0 + i - DW_K / 2;
        xs[i] = (t >= 0 && t < T) ? x[base + (int64_t)t * C + c] : 0.f;
    }
    const float bc = bias[c];
    // two outputs at a time through the branch-free GELU of the GEMM epilogues (1-ulp erf, packed fp32): the library erff was
    // two thirds of this kernel's VALU work
#pragma unroll
    for (int o = 0; o < DW_TT; o += 2) {
        float a0 = bc, a1 = bc;
#pragma unroll
        for (int k = 0; k < DW_K; ++k) { a0 = fmaf(wk[k], xs[o + k], a0); a1 = fmaf(wk[k], xs[o + 1 + k], a1); }
        const f32x2 g2 = gelu_fast2(f32x2{a0, a1});
        const int t = t0 + o;
        if (t < T) y[base + (int64_t)t * C + c] = g2[0] + xs[o + DW_K / 2];
        if (t + 1 < T) y[base + (int64_t)(t + 1) * C + c] = g2[1] + xs[o + 1 + DW_K / 2];
    }
}

// ---------------------------------------------------------------- skinny GEMM: C[M <= 32][N] = A[M][K] . W[N][K]^T (+ bias)
// A product with a handful of rows is weight streaming (the adaptive-norm table of a solve - 32 evaluation times x 32,768
// outputs, K = 4,096 - took 1.35 ms on the tiled fp32 kernel and 0.79 ms on the split-precision one: 537 MB of weights for 8.6
// GFLOP).  Here every wave owns tiles of 32 W rows: lane (r, g) streams 16-byte pieces of ITS row (non-temporal, SK_Q steps
// requested ahead in registers), all M rows of A sit in LDS ([m][K + 4] fp32: conflict-free b128 reads), and the tile is
// 32 x 32 outputs of v_mfma_f32_32x32x2_f32 - exact fp32 products; one 16-byte piece of W and of A feeds four MFMAs, the K
// order being permuted consistently in both operands (lanes g = 0 / 1 take k = 8q + j / 8q + 4 + j in step j).
constexpr int SK_M = 32;
constexpr int SK_KC = 1024;                    // columns of A staged in LDS at a time (longer K: chunk by chunk, accumulators stay)
constexpr int SK_Q = 16;                        // K steps (of 8) requested ahead: 16 x 4 MFMAs = 4096 matrix cycles per round trip
__global__ __launch_bounds__(256) void gemm_skinny_kernel(const float* __restrict__ A, int lda, const float* __restrict__ W, int64_t ldw,
                                                         const float* __restrict__ bias, float* __restrict__ Cm, int64_t ldc,
                                                         int M, int N, int K, int act)
{
    extern __shared__ __attribute__((aligned(16))) float sk_a[];          // [SK_M][KC + 4] (one K chunk of A), rows >= M zero
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int KC = min(K, SK_KC), ldA = KC + 4;
    const int i31 = lane & 31, g = lane >> 5;
    const float* ar = sk_a + (size_t)i31 * ldA + 4 * g;                   // this lane's A row (m = i31), its half of every 8 k
    const int n_tiles = (N + 31) / 32;
    for (int tile0 = blockIdx.x * 4; tile0 < n_tiles; tile0 += gridDim.x * 4) {       // (block-uniform: the chunk staging has barriers)
        const int tile = tile0 + wid;
        const bool active = tile < n_tiles;
        const int n0 = tile * 32;
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
        for (int kc = 0; kc < K; kc += KC) {
            const int kn = min(KC, K - kc), k4 = kn >> 2, nq = kn >> 3;  // K % 8 == 0
            __syncthreads();                                              // the previous chunk (or tile round) is consumed
            for (int i = tid; i < SK_M * k4; i += 256) {
                const int m = i / k4, c = i - m * k4;
                *reinterpret_cast<f32x4*>(sk_a + (size_t)m * ldA + 4 * c) = m < M ? gload4(A + (size_t)m * lda + kc + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            __syncthreads();
            if (!active) continue;
            const float* wr = W + (int64_t)min(n0 + i31, N - 1) * ldw + kc + 4 * g;
            f32x4 wb[2][SK_Q];
#pragma unroll
            for (int u = 0; u < SK_Q; ++u) wb[0][u] = u < nq ? gload4_nt(wr + 8 * u) : f32x4{0.f, 0.f, 0.f, 0.f};
            for (int q0 = 0; q0 < nq; q0 += 2 * SK_Q) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int qb = q0 + half * SK_Q;
                    if (qb < nq) {
#pragma unroll
                        for (int u = 0; u < SK_Q; ++u)                    // the next SK_Q pieces of the row
                            wb[half ^ 1][u] = qb + SK_Q + u < nq ? gload4_nt(wr + 8 * (qb + SK_Q + u)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int u = 0; u < SK_Q; ++u) {
                            if (qb + u < nq) {
                                const f32x4 av = *reinterpret_cast<const f32x4*>(ar + 8 * (qb + u));
                                const f32x4 wv = wb[half][u];
                                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[0], av[0], acc0, 0, 0, 0);
                                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[1], av[1], acc1, 0, 0, 0);
                                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[2], av[2], acc0, 0, 0, 0);
                                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[3], av[3], acc1, 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
        if (!active) continue;
        // acc[r]: W row n0 + (r & 3) + 8 (r >> 2) + 4 g, A row m = i31
        if (i31 < M) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + (r & 3) + 8 * (r >> 2) + 4 * g;
                if (n < N) {
                    float v = acc0[r] + acc1[r];
                    if (bias) v += bias[n];
                    if (act == CVX_ACT_SILU) v = silu(v);
                    else if (act == CVX_ACT_GELU) v = gelu_erf(v);
                    else if (act == CVX_ACT_TANH) v = tanhf(v);
                    Cm[(int64_t)i31 * ldc + n] = v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------- CFG combine + axpy
__global__ __launch_bounds__(256) void cfg_axpy_kernel(const float* __restrict__ fc, const float* __restrict__ fn,
                                                      const float* y, float s, float coef,   // out may alias y
                                                      float* out, float* __restrict__ out2,
                                                      float* __restrict__ out3, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = fc[i];
    if (fn) v = v * (1.0f + s) - s * fn[i];
    const float o = y[i] + v * coef;
    out[i] = o;
    if (out2) out2[i] = o;
    if (out3) out3[i] = o;
}

// ---------------------------------------------------------------- CFG combine + one stage of an explicit Runge-Kutta step
// cfg_axpy_kernel's combine and update, verbatim (same expressions, same contraction: with no stored stage, no k_out and no
// row scales the bits are that kernel's), plus up to three stored stages, a per-row guidance scale and the combined field as
// an output.  wk[j] of an unused or zero-weight stage is 0: such a stage is neither read nor added.
struct RkStage {
    const float* fc; const float* fn; const float* y; const float* row_scale;
    const float* k0; const float* k1; const float* k2;
    float wk0, wk1, wk2, wv, s;
    float* k_out; float* out; float* out2; float* out3;          // out may alias y
    int64_t n;
    int dim;
};

// cfg_axpy_kernel's arithmetic as its gfx950 code has it (v_pk_mul_f32, v_sub_f32, v_fmac_f32): the two products of the combine are
// rounded on their own and subtracted, the update is one fused multiply-add.  Spelled out, because the compiler contracts the
// plain expressions differently from one lane of a float4 to the next.
__device__ __forceinline__ float rk_cfg_combine(float v, float f, float s)
{
#pragma clang fp contract(off)
    const float a = v * (1.0f + s), b = s * f;
    return a - b;
}

// KEEP (the error-estimate kernel): vo receives the combined field of the V elements from i0, then their new state (what `out` receives)
template <int V, bool KEEP = false>
__device__ __forceinline__ void rk_stage_elems(const RkStage& a, int64_t i0, float* vo = nullptr)
{
    float v[V], o[V];
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(a.fc + i0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else v[0] = a.fc[i0];
    if (a.fn) {
        float f[V], s[V];
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(a.fn + i0);
            f[0] = t.x; f[1] = t.y; f[2] = t.z; f[3] = t.w;
        } else f[0] = a.fn[i0];
        if (a.row_scale) {
            int64_t r = i0 / a.dim;
            int rem = (int)(i0 - r * a.dim);
#pragma unroll
            for (int e = 0; e < V; ++e) {                           // (element i0 + e < n: its row is inside the table)
                s[e] = a.row_scale[r];
                if (++rem == a.dim) { rem = 0; ++r; }
            }
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (s[e] != 1.0f) v[e] = rk_cfg_combine(v[e], f[e], s[e]);   // a row at exactly 1.0 takes f_c (acoustic.py:423)
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = rk_cfg_combine(v[e], f[e], a.s);
        }
    }
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(a.y + i0);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else o[0] = a.y[i0];
    if (a.k_out) {
        if constexpr (V == 4) *reinterpret_cast<float4*>(a.k_out + i0) = make_float4(v[0], v[1], v[2], v[3]);
        else a.k_out[i0] = v[0];
    }
#define RK_ADD_STAGE(K, W)                                                              \
    if ((W) != 0.f) {                                                                   \
        if constexpr (V == 4) {                                                         \
            const float4 t = *reinterpret_cast<const float4*>((K) + i0);                \
            o[0] = __builtin_fmaf(t.x, (W), o[0]); o[1] = __builtin_fmaf(t.y, (W), o[1]);   \
            o[2] = __builtin_fmaf(t.z, (W), o[2]); o[3] = __builtin_fmaf(t.w, (W), o[3]);   \
        } else o[0] = __builtin_fmaf((K)[i0], (W), o[0]);                               \
    }
    RK_ADD_STAGE(a.k0, a.wk0)
    RK_ADD_STAGE(a.k1, a.wk1)
    RK_ADD_STAGE(a.k2, a.wk2)
#undef RK_ADD_STAGE
    if (a.wv != 0.f) {
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = __builtin_fmaf(v[e], a.wv, o[e]);
    }
    if constexpr (V == 4) {
        const float4 t = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(a.out + i0) = t;
        if (a.out2) *reinterpret_cast<float4*>(a.out2 + i0) = t;
        if (a.out3) *reinterpret_cast<float4*>(a.out3 + i0) = t;
    } else {
        a.out[i0] = o[0];
        if (a.out2) a.out2[i0] = o[0];
        if (a.out3) a.out3[i0] = o[0];
    }
    if constexpr (KEEP) {
#pragma unroll
        for (int e = 0; e < V; ++e) { vo[e] = v[e]; vo[V + e] = o[e]; }
    }
}

// V = 4: every base pointer is 16-byte aligned - one float4 per lane, the last n % 4 elements one at a time; V = 1 otherwise
template <int V>
__global__ __launch_bounds__(256) void rk_stage_kernel(const RkStage a)
{
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (i0 >= a.n) return;
    if (V == 1 || i0 + V <= a.n) { rk_stage_elems<V>(a, i0); return; }
    for (int64_t i = i0; i < a.n; ++i) rk_stage_elems<1>(a, i);
}

// ---------------------------------------------------------------- the last stage of a step + the embedded error estimate
// rk_stage_elems on a block's chunk of rows, plus per element delta = sum_j k_j we_j (stored stages first, in j order, then this
// launch's v; a zero weight is neither read nor added; the first term is fma(k, we, 0) = the rounded product) and the two sums
// of squares.  A block owns one chunk of at most CVX_RK_ERR_ROWS consecutive rows of ONE sequence, counted from that sequence's
// first row: thread t takes the chunk's elements (t + 256 i) V ... in i order, so what a thread adds, and in which order, depends on
// the chunk's own rows only - not on where the sequence lies in the batch.  Lane sums (wave_sum), then the four waves in wave order
// through LDS: one fixed tree, no atomics.
struct RkErr {
    const float* e0; const float* e1; const float* e2;
    float we0, we1, we2, wev;
    const int32_t* map;          // per block: first row, rows, sequence
    float2* partials;            // per block: (sum delta^2, sum o^2)
};

template <int V>
__device__ __forceinline__ void rk_err_elems(const RkStage& a, const RkErr& e, int64_t i0, float& sd, float& so)
{
    float vo[2 * V], d[V];
    rk_stage_elems<V, true>(a, i0, vo);
    const float *v = vo, *o = vo + V;
#pragma unroll
    for (int l = 0; l < V; ++l) d[l] = 0.f;
#define RK_ERR_STAGE(K, W)                                                              \
    if ((W) != 0.f) {                                                                   \
        if constexpr (V == 4) {                                                         \
            const float4 t = *reinterpret_cast<const float4*>((K) + i0);                \
            d[0] = __builtin_fmaf(t.x, (W), d[0]); d[1] = __builtin_fmaf(t.y, (W), d[1]);   \
            d[2] = __builtin_fmaf(t.z, (W), d[2]); d[3] = __builtin_fmaf(t.w, (W), d[3]);   \
        } else d[0] = __builtin_fmaf((K)[i0], (W), d[0]);                               \
    }
    RK_ERR_STAGE(e.e0, e.we0)
    RK_ERR_STAGE(e.e1, e.we1)
    RK_ERR_STAGE(e.e2, e.we2)
#undef RK_ERR_STAGE
    if (e.wev != 0.f) {
#pragma unroll
        for (int l = 0; l < V; ++l) d[l] = __builtin_fmaf(v[l], e.wev, d[l]);
    }
#pragma unroll
    for (int l = 0; l < V; ++l) {
        sd = __builtin_fmaf(d[l], d[l], sd);
        so = __builtin_fmaf(o[l], o[l], so);
    }
}

// V = 4: every base pointer is 16-byte aligned and dim % 4 == 0 (every chunk then starts and ends on a float4); V = 1 otherwise
template <int V>
__global__ __launch_bounds__(256) void rk_err_stage_kernel(const RkStage a, const RkErr e)
{
    __shared__ float red[8];
    const int32_t* mp = e.map + 3 * (int64_t)blockIdx.x;
    const int64_t base = (int64_t)mp[0] * a.dim;
    const int64_t cnt = (base >= 0 && base < a.n) ? ((int64_t)mp[1] * a.dim < a.n - base ? (int64_t)mp[1] * a.dim : a.n - base) : 0;   // (never past the launch's rows)
    float sd = 0.f, so = 0.f;
    for (int64_t i = (int64_t)threadIdx.x * V; i < cnt; i += 256 * V) rk_err_elems<V>(a, e, base + i, sd, so);
    sd = wave_sum(sd);
    so = wave_sum(so);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave] = sd; red[4 + wave] = so; }
    __syncthreads();
    if (threadIdx.x == 0)
        e.partials[blockIdx.x] = make_float2(((red[0] + red[1]) + red[2]) + red[3], ((red[4] + red[5]) + red[6]) + red[7]);
}

// one thread per (step, sequence): the chunk sums of the blocks the map gives to that sequence, in block order
__global__ __launch_bounds__(256) void rk_err_finish_kernel(const float2* __restrict__ partials, const int32_t* __restrict__ map,
                                                            float2* __restrict__ err, int steps, int n_seq, int blocks)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= steps * n_seq) return;
    const int step = i / n_seq, q = i - step * n_seq;
    const float2* p = partials + (int64_t)step * blocks;
    float sd = 0.f, so = 0.f;
    for (int b = 0; b < blocks; ++b)
        if (map[3 * b + 2] == q) { sd += p[b].x; so += p[b].y; }
    err[i] = make_float2(sd, so);
}

// ---------------------------------------------------------------- embedding gather
__global__ __launch_bounds__(256) void embed_gather_kernel(const int64_t* __restrict__ ids, int S,
                                                          const float* __restrict__ table, int E, int n_rows_table,
                                                          const float* __restrict__ cond, const float* __restrict__ cond_row,
                                                          int Cc, int64_t null_id, float* __restrict__ out)
{
    const int64_t m = blockIdx.x;
    const int width = S * E + Cc;
    float* o = out + m * width;
    for (int j = threadIdx.x; j < width; j += 256) {
        float v;
        if (j < S * E) {
            const int s = j / E, e = j - s * E;
            int64_t id = ids ? ids[m * S + s] : null_id;
            id = id < 0 ? 0 : (id >= n_rows_table ? n_rows_table - 1 : id);
            v = table[id * E + e];
        } else {
            const int cidx = j - S * E;
            v = cond_row ? cond_row[cidx] : cond[m * Cc + cidx];
        }
        o[j] = v;
    }
}

// ---------------------------------------------------------------- time Fourier features
__global__ __launch_bounds__(256) void time_fourier_kernel(const float* __restrict__ times, const float* __restrict__ w,
                                                          float* __restrict__ out, int half)
{
    const int i = blockIdx.x;
    const float t = times[i];
    for (int j = threadIdx.x; j < half; j += 256) {
        const float ang = t * w[j] * 2.0f * 3.14159265358979323846f;
        out[(int64_t)i * 2 * half + j] = sinf(ang);
        out[(int64_t)i * 2 * half + half + j] = cosf(ang);
    }
}

// ---------------------------------------------------------------- float wav -> int16 PCM
__global__ __launch_bounds__(256) void wav_to_int16_kernel(const float* __restrict__ wav, int16_t* __restrict__ pcm, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = wav[i] * 32768.0f;
    pcm[i] = (int16_t)(int32_t)v;     // trunc toward zero, wrap like numpy astype on x86
}

// ---------------------------------------------------------------- prompt mel extraction (row N3) epilogues
// spec [T, 2*nb] = (re | im) of the windowed DFT  ->  mag [T, nbp] = sqrt(re^2 + im^2 + 1e-9), zero in the padding
__global__ __launch_bounds__(256) void mel_magnitude_kernel(const float* __restrict__ spec, float* __restrict__ mag,
                                                           int64_t T, int nb, int nbp)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * nbp) return;
    const int64_t t = i / nbp;
    const int k = (int)(i - t * nbp);
    float v = 0.f;
    if (k < nb) {
        const float re = spec[t * 2 * nb + k], im = spec[t * 2 * nb + nb + k];
        v = sqrtf(re * re + im * im + 1e-9f);
    }
    mag[i] = v;
}

// x [T, n_mels] -> y [n_mels, T] = log(max(x, 1e-5))
__global__ __launch_bounds__(256) void mel_log_transpose_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t T, int n_mels)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * n_mels) return;
    const int m = (int)(i / T);
    const int64_t t = i - (int64_t)m * T;
    y[i] = logf(fmaxf(x[t * n_mels + m], 1e-5f));
}

}  // namespace

extern "C" int cvx_mel_magnitude_f32(const float* spec, float* mag, int64_t T, int32_t nb, int32_t nbp, cvx_stream_t s)
{
    CVX_REQUIRE(spec && mag && T >= 0 && nb > 0 && nbp >= nb, "mel_magnitude: bad arguments");
    if (T == 0) return CVX_OK;
    hipLaunchKernelGGL(mel_magnitude_kernel, dim3((unsigned)((T * nbp + 255) / 256)), dim3(256), 0, cvx_hip_stream(s),
                       spec, mag, T, nb, nbp);
    CVX_CHECK_LAUNCH("cvx_mel_magnitude_f32");
    return CVX_OK;
}

extern "C" int cvx_mel_log_transpose_f32(const float* x, float* y, int64_t T, int32_t n_mels, cvx_stream_t s)
{
    CVX_REQUIRE(x && y && T >= 0 && n_mels > 0, "mel_log_transpose: bad arguments");
    if (T == 0) return CVX_OK;
    hipLaunchKernelGGL(mel_log_transpose_kernel, dim3((unsigned)((T * n_mels + 255) / 256)), dim3(256), 0,
                       cvx_hip_stream(s), x, y, T, n_mels);
    CVX_CHECK_LAUNCH("cvx_mel_log_transpose_f32");
    return CVX_OK;
}

extern "C" int cvx_adarmsnorm_scaled_f32(const float* x, const float* gamma, const float* beta, float* y,
                                  uint16_t* y_hi_, uint16_t* y_lo_,
                                  int64_t rows, int32_t D, int64_t rows_per_group, float scale, float eps,
                                  const float* split_scale_dev, cvx_stream_t s)
{
    CVX_REQUIRE(x && gamma && (y || y_hi_) && (y_hi_ || !y_lo_), "adarmsnorm: null pointer");     // y_lo == NULL: hi halves only
    _Float16* y_hi = reinterpret_cast<_Float16*>(y_hi_);
    _Float16* y_lo = reinterpret_cast<_Float16*>(y_lo_);
    CVX_REQUIRE(rows >= 0 && D > 0 && D % 4 == 0 && rows_per_group > 0, "adarmsnorm: bad shape rows=%ld D=%d", (long)rows, D);
    // interleaved pair: store_split4 maps the flat offset row * D + col, which is the row's own line only when D % 32 == 0
    CVX_REQUIRE(!(y_hi && y_lo == y_hi + 32) || D % 32 == 0, "adarmsnorm: an interleaved pair (y_lo == y_hi + 32) needs D %% 32 == 0 (D=%d)", D);
    if (rows == 0) return CVX_OK;
    hipStream_t st = cvx_hip_stream(s);
    dim3 grid((unsigned)((rows + 3) / 4));
    if (y_hi) CVX_REQUIRE_SAT(s);
    uint32_t* sat = y_hi ? cvx_sat_flag_for(s) : nullptr;
    if (D <= 256)       hipLaunchKernelGGL(adarmsnorm_kernel<1>, grid, dim3(256), 0, st, x, gamma, beta, y, y_hi, y_lo, rows, D, rows_per_group, scale, eps, split_scale_dev, sat);
    else if (D <= 512)  hipLaunchKernelGGL(adarmsnorm_kernel<2>, grid, dim3(256), 0, st, x, gamma, beta, y, y_hi, y_lo, rows, D, rows_per_group, scale, eps, split_scale_dev, sat);
    else if (D <= 1024) hipLaunchKernelGGL(adarmsnorm_kernel<4>, grid, dim3(256), 0, st, x, gamma, beta, y, y_hi, y_lo, rows, D, rows_per_group, scale, eps, split_scale_dev, sat);
    else                hipLaunchKernelGGL(adarmsnorm_generic_kernel, grid, dim3(256), 0, st, x, gamma, beta, y, y_hi, y_lo, rows, D, rows_per_group, scale, eps, split_scale_dev, sat);
    CVX_CHECK_LAUNCH("cvx_adarmsnorm_scaled_f32");
    return CVX_OK;
}

extern "C" int cvx_adarmsnorm_f32(const float* x, const float* gamma, const float* beta, float* y,
                                  uint16_t* y_hi, uint16_t* y_lo,
                                  int64_t rows, int32_t D, int64_t rows_per_group, float scale, float eps,
                                  cvx_stream_t s)
{
    return cvx_adarmsnorm_scaled_f32(x, gamma, beta, y, y_hi, y_lo, rows, D, rows_per_group, scale, eps, nullptr, s);
}

// ---------------------------------------------------------------- deferred norm: per-row factor from a producer GEMM's partial sums
// (cvx_gemm_split_io.c_rowsq: one sum of squares per 64-column slice of a row; reference acoustic.py:198-204, F.normalize's eps)
namespace {
__global__ __launch_bounds__(256) void rownorm_scale_kernel(const float* __restrict__ rowsq, int64_t rows, int parts, int64_t ld,
                                                            float scale, float eps, float* __restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float* p = rowsq + r * ld;
    float q = 0.f;
    if ((parts & 3) == 0 && (ld & 3) == 0) {
        for (int j = 0; j < parts; j += 4) { const f32x4 v = gload4(p + j); q += v[0]; q += v[1]; q += v[2]; q += v[3]; }
    } else {
        for (int j = 0; j < parts; ++j) q += p[j];
    }
    out[r] = scale / fmaxf(sqrtf(q), eps);
}
}  // namespace

extern "C" int cvx_rownorm_scale_f32(const float* rowsq, int64_t rows, int32_t parts, int64_t ld, float scale, float eps, float* out, cvx_stream_t s)
{
    CVX_REQUIRE(rowsq && out && rows >= 0 && parts > 0 && parts <= 64 && ld >= parts && (((uintptr_t)rowsq & 15) == 0 || (parts & 3) || (ld & 3)),
                "rownorm_scale: bad arguments (rows=%ld parts=%d ld=%ld)", (long)rows, parts, (long)ld);
    if (rows == 0) return CVX_OK;
    hipLaunchKernelGGL(rownorm_scale_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, cvx_hip_stream(s),
                       rowsq, rows, parts, ld, scale, eps, out);
    CVX_CHECK_LAUNCH("cvx_rownorm_scale_f32");
    return CVX_OK;
}

// ---------------------------------------------------------------- measured power-of-two pre-scale of a tensor
namespace {
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, int64_t n, unsigned* __restrict__ amax_bits)
{
    // four independent 16-byte loads per thread and trip; ONE atomic per block, and only from blocks that can still raise the
    // maximum (2048 x 4 same-address atomics used to be most of this kernel: 100 us for 164 MB)
    __shared__ float part[4];
    float m = 0.f;
    const int64_t n4 = n / 4, stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = gload4(x + 4 * (i + u * stride));
#pragma unroll
        for (int u = 0; u < 4; ++u) m = fmaxf(m, fmaxf(fmaxf(fabsf(v[u][0]), fabsf(v[u][1])), fmaxf(fabsf(v[u][2]), fabsf(v[u][3]))));
    }
    for (; i < n4; i += stride) {
        const f32x4 v = gload4(x + 4 * i);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = fmaxf(m, fabsf(x[4 * n4 + threadIdx.x]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
        if (m > 0.f && m < __builtin_inff() && __float_as_uint(m) > __atomic_load_n(amax_bits, __ATOMIC_RELAXED))
            atomicMax(amax_bits, __float_as_uint(m));        // non-negative floats order like their bits
    }
}
__global__ void pow2_scale_kernel(const unsigned* __restrict__ amax_bits, float target, float* __restrict__ scale)
{
    const float a = __uint_as_float(*amax_bits);
    float e = 0.f;
    if (a > 0.f) e = fminf(fmaxf(rintf(log2f(target / a)), -40.f), 40.f);
    *scale = exp2f(e);
}
}  // namespace

extern "C" int cvx_amax_pow2_scale_f32(const float* x, int64_t n, float target, float* scale_dev, uint32_t* scratch_dev, cvx_stream_t s)
{
    CVX_REQUIRE(x && scale_dev && scratch_dev && n >= 0 && target > 0.f && ((uintptr_t)x & 15) == 0, "amax_pow2_scale: bad arguments");
    hipStream_t st = cvx_hip_stream(s);
    if (hipMemsetAsync(scratch_dev, 0, sizeof(uint32_t), st) != hipSuccess) { cvx_set_error("amax_pow2_scale: memset failed"); return CVX_EHIP; }
    if (n > 0) {
        const unsigned blocks = (unsigned)((n / 4 + 1023) / 1024 < 2048 ? (n / 4 + 1023) / 1024 + 1 : 2048);
        hipLaunchKernelGGL(amax_kernel, dim3(blocks), dim3(256), 0, st, x, n, scratch_dev);
    }
    hipLaunchKernelGGL(pow2_scale_kernel, dim3(1), dim3(1), 0, st, scratch_dev, target, scale_dev);
    // leave the scratch word ZERO, as cvx_pow2_scale_from_amax_f32 does: a producer kernel that max-accumulates into the same word
    // afterwards (the vocoder's upsampler of the NEXT call) must not see this call's maximum (round 4: it did - the first call of
    // a shape and the later ones differed by an fp32 rounding, and a call's scale depended on the previous call's input)
    if (hipMemsetAsync(scratch_dev, 0, sizeof(uint32_t), st) != hipSuccess) { cvx_set_error("amax_pow2_scale: memset failed"); return CVX_EHIP; }
    CVX_CHECK_LAUNCH("cvx_amax_pow2_scale_f32");
    return CVX_OK;
}

extern "C" int cvx_pow2_scale_from_amax_f32(uint32_t* amax_bits_dev, float target, float* scale_dev, cvx_stream_t s)
{
    CVX_REQUIRE(amax_bits_dev && scale_dev && target > 0.f, "pow2_scale_from_amax: bad arguments");
    hipStream_t st = cvx_hip_stream(s);
    hipLaunchKernelGGL(pow2_scale_kernel, dim3(1), dim3(1), 0, st, amax_bits_dev, target, scale_dev);
    if (hipMemsetAsync(amax_bits_dev, 0, sizeof(uint32_t), st) != hipSuccess) { cvx_set_error("pow2_scale_from_amax: memset failed"); return CVX_EHIP; }
    CVX_CHECK_LAUNCH("cvx_pow2_scale_from_amax_f32");
    return CVX_OK;
}

extern "C" int cvx_dwconv31_gelu_res_varlen_f32(const float* x, const float* w, const float* bias, float* y,
                                                const int32_t* cu_seqlens_dev, int32_t Bt, int32_t max_T, int32_t C, cvx_stream_t s)
{
    CVX_REQUIRE(x && w && bias && y, "dwconv31: null pointer");
    CVX_REQUIRE(Bt >= 0 && max_T > 0 && C > 0 && Bt <= 65535, "dwconv31: bad shape");
    CVX_REQUIRE(x != y, "dwconv31: in-place operation is not supported");
    if (Bt == 0) return CVX_OK;
    dim3 grid((C + 255) / 256, (max_T + DW_TT - 1) / DW_TT, Bt);
    hipLaunchKernelGGL(dwconv31_kernel, grid, dim3(256), 0, cvx_hip_stream(s), x, w, bias, y, max_T, C, cu_seqlens_dev);
    CVX_CHECK_LAUNCH("cvx_dwconv31_gelu_res_f32");
    return CVX_OK;
}

extern "C" int cvx_gemm_skinny_f32(const float* A, int32_t lda, const float* W, int64_t ldw, const float* bias, float* C, int64_t ldc,
                                   int32_t M, int32_t N, int32_t K, int32_t act, cvx_stream_t s)
{
    CVX_REQUIRE(A && W && C && M >= 0 && M <= SK_M && N >= 0 && K > 0 && K % 8 == 0 && lda >= K && lda % 4 == 0 && ldw >= K &&
                ldw % 4 == 0 && ldc >= N && act >= CVX_ACT_NONE && act <= CVX_ACT_TANH,
                "gemm_skinny: M <= 32, K a multiple of 8, lda / ldw multiples of 4 (M=%d N=%d K=%d)", M, N, K);
    CVX_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0, "gemm_skinny: 16-byte aligned operands");
    if (M == 0 || N == 0) return CVX_OK;
    const size_t lds = (size_t)SK_M * (std::min(K, SK_KC) + 4) * sizeof(float);
    cvx_allow_dynamic_lds(reinterpret_cast<const void*>(&gemm_skinny_kernel), (int)lds);
    const int64_t groups = ((int64_t)N + 127) / 128;                       // four 32-row tiles per block and trip
    const unsigned grid = (unsigned)std::min<int64_t>(groups, (int64_t)cvx_ctx_cus(s));
    hipLaunchKernelGGL(gemm_skinny_kernel, dim3(grid), dim3(256), lds, cvx_hip_stream(s), A, lda, W, ldw, bias, C, ldc, M, N, K, act);
    CVX_CHECK_LAUNCH("cvx_gemm_skinny_f32");
    return CVX_OK;
}

extern "C" int cvx_dwconv31_gelu_res_f32(const float* x, const float* w, const float* bias, float* y,
                                         int32_t Bt, int32_t T, int32_t C, cvx_stream_t s)
{
    return cvx_dwconv31_gelu_res_varlen_f32(x, w, bias, y, nullptr, Bt, T, C, s);
}

extern "C" int cvx_cfg_combine_axpy_f32(const float* f_c, const float* f_n, const float* y, float cond_scale,
                                        float coef, float* out, float* out2, float* out3, int64_t n, cvx_stream_t s)
{
    CVX_REQUIRE(f_c && y && out && n >= 0, "cfg_axpy: bad arguments");
    if (n == 0) return CVX_OK;
    hipLaunchKernelGGL(cfg_axpy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cvx_hip_stream(s),
                       f_c, f_n, y, cond_scale, coef, out, out2, out3, n);
    CVX_CHECK_LAUNCH("cvx_cfg_combine_axpy_f32");
    return CVX_OK;
}

// the argument checks of both stage entry points; *vec: every pointer of the launch is 16-byte aligned
static int rk_stage_args(RkStage& a, bool* vec, const float* f_c, const float* f_n, const float* y, float cond_scale, const float* row_scale,
                         const float* const* k_prev, const float* w, int32_t m, float* k_out, float* out, float* out2, float* out3,
                         int64_t rows, int32_t dim)
{
    CVX_REQUIRE(f_c && y && out && w, "rk_stage: f_c, y, out and w must not be null");
    CVX_REQUIRE(m >= 0 && m <= 3, "rk_stage: at most 3 stored stages (m=%d)", m);
    CVX_REQUIRE(rows >= 0 && dim > 0, "rk_stage: bad shape (rows=%lld dim=%d)", (long long)rows, dim);
    CVX_REQUIRE(!row_scale || f_n, "rk_stage: row_scale without f_n");
    CVX_REQUIRE(m == 0 || k_prev, "rk_stage: k_prev is null");
    const float* k[3] = {nullptr, nullptr, nullptr};
    float wk[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < m; ++j) {
        CVX_REQUIRE(k_prev[j] || w[j] == 0.f, "rk_stage: k_prev[%d] is null and its weight is not 0", j);
        if (w[j] != 0.f) { k[j] = k_prev[j]; wk[j] = w[j]; }
    }
    CVX_REQUIRE(rows <= (int64_t)0x7fffffffffffLL / dim, "rk_stage: rows x dim too large");
    a.fc = f_c; a.fn = f_n; a.y = y; a.row_scale = row_scale;
    a.k0 = k[0]; a.k1 = k[1]; a.k2 = k[2];
    a.wk0 = wk[0]; a.wk1 = wk[1]; a.wk2 = wk[2]; a.wv = w[m]; a.s = cond_scale;
    a.k_out = k_out; a.out = out; a.out2 = out2; a.out3 = out3;
    a.n = rows * dim; a.dim = dim;
    uintptr_t bits = (uintptr_t)f_c | (uintptr_t)f_n | (uintptr_t)y | (uintptr_t)k[0] | (uintptr_t)k[1] | (uintptr_t)k[2] |
                     (uintptr_t)k_out | (uintptr_t)out | (uintptr_t)out2 | (uintptr_t)out3;
    *vec = (bits & 15) == 0;
    return CVX_OK;
}

extern "C" int cvx_rk_stage_f32(const float* f_c, const float* f_n, const float* y, float cond_scale, const float* row_scale,
                                const float* const* k_prev, const float* w, int32_t m, float* k_out, float* out, float* out2,
                                float* out3, int64_t rows, int32_t dim, cvx_stream_t s)
{
    RkStage a = {};
    bool vec = false;
    const int rc = rk_stage_args(a, &vec, f_c, f_n, y, cond_scale, row_scale, k_prev, w, m, k_out, out, out2, out3, rows, dim);
    if (rc != CVX_OK) return rc;
    if (a.n == 0) return CVX_OK;
    const int64_t threads = vec ? (a.n + 3) / 4 : a.n;
    const int64_t blocks = (threads + 255) / 256;
    CVX_REQUIRE(blocks <= 0x7fffffffLL, "rk_stage: rows x dim too large for one launch");
    if (vec) hipLaunchKernelGGL(rk_stage_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, cvx_hip_stream(s), a);
    else hipLaunchKernelGGL(rk_stage_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, cvx_hip_stream(s), a);
    CVX_CHECK_LAUNCH("cvx_rk_stage_f32");
    return CVX_OK;
}

extern "C" int cvx_rk_stage_err_f32(const float* f_c, const float* f_n, const float* y, float cond_scale, const float* row_scale,
                                    const float* const* k_prev, const float* w, const float* we, int32_t m, float* k_out, float* out,
                                    float* out2, float* out3, int64_t rows, int32_t dim, const int32_t* map_dev, const int32_t* map_host,
                                    int32_t blocks, float* partials, cvx_stream_t s)
{
    RkStage a = {};
    bool vec = false;
    const int rc = rk_stage_args(a, &vec, f_c, f_n, y, cond_scale, row_scale, k_prev, w, m, k_out, out, out2, out3, rows, dim);
    if (rc != CVX_OK) return rc;
    CVX_REQUIRE(we && map_dev && map_host && partials, "rk_stage_err: we, the map (device and host copy) and partials must not be null");
    CVX_REQUIRE(((uintptr_t)map_dev & 3) == 0 && ((uintptr_t)partials & 7) == 0, "rk_stage_err: map 4-byte, partials 8-byte aligned");
    CVX_REQUIRE(blocks >= 0 && rows <= 0x7fffffffLL, "rk_stage_err: bad block count %d / rows beyond int32", blocks);
    RkErr e = {};
    const float* k[3] = {nullptr, nullptr, nullptr};
    float wk[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < m; ++j) {
        CVX_REQUIRE(k_prev[j] || we[j] == 0.f, "rk_stage_err: k_prev[%d] is null and its error weight is not 0", j);
        if (we[j] != 0.f) { k[j] = k_prev[j]; wk[j] = we[j]; }
    }
    // the chunks must tile [0, rows) in order, each 1 .. CVX_RK_ERR_ROWS rows of one sequence, sequences in ascending order; a chunk
    // shorter than CVX_RK_ERR_ROWS ends its sequence (chunks are counted from a sequence's first row)
    int64_t next = 0;
    for (int b = 0; b < blocks; ++b) {
        const int32_t r0 = map_host[3 * b], nr = map_host[3 * b + 1], q = map_host[3 * b + 2];
        CVX_REQUIRE(r0 == next && nr >= 1 && nr <= CVX_RK_ERR_ROWS && q >= 0, "rk_stage_err: map entry %d (first row %d, rows %d, sequence %d) "
                    "does not continue at row %lld with 1..%d rows", b, r0, nr, q, (long long)next, CVX_RK_ERR_ROWS);
        if (b > 0) {
            const int32_t pq = map_host[3 * b - 1], pn = map_host[3 * b - 2];
            CVX_REQUIRE(q == pq ? pn == CVX_RK_ERR_ROWS : q > pq, "rk_stage_err: map entry %d: sequence %d after %d (a short chunk ends its sequence)", b, q, pq);
        }
        next += nr;
    }
    CVX_REQUIRE(next == rows, "rk_stage_err: the map covers %lld rows, the launch has %lld", (long long)next, (long long)rows);
    if (a.n == 0) return CVX_OK;
    e.e0 = k[0]; e.e1 = k[1]; e.e2 = k[2];
    e.we0 = wk[0]; e.we1 = wk[1]; e.we2 = wk[2]; e.wev = we[m];
    e.map = map_dev; e.partials = reinterpret_cast<float2*>(partials);
    vec = vec && (((uintptr_t)k[0] | (uintptr_t)k[1] | (uintptr_t)k[2]) & 15) == 0 && dim % 4 == 0;
    if (vec) hipLaunchKernelGGL(rk_err_stage_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, cvx_hip_stream(s), a, e);
    else hipLaunchKernelGGL(rk_err_stage_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, cvx_hip_stream(s), a, e);
    CVX_CHECK_LAUNCH("cvx_rk_stage_err_f32");
    return CVX_OK;
}

extern "C" int cvx_rk_err_finish_f32(const float* partials, const int32_t* map_dev, int32_t blocks, int32_t steps, int32_t n_seq, float* err,
                                     cvx_stream_t s)
{
    CVX_REQUIRE(partials && map_dev && err, "rk_err_finish: partials, map and err must not be null");
    CVX_REQUIRE(((uintptr_t)partials & 7) == 0 && ((uintptr_t)err & 7) == 0 && ((uintptr_t)map_dev & 3) == 0, "rk_err_finish: 8-byte aligned partials and err");
    CVX_REQUIRE(blocks >= 0 && steps >= 0 && n_seq >= 0 && (int64_t)steps * n_seq <= 0x7fffffffLL && (int64_t)steps * blocks <= 0x7fffffffLL,
                "rk_err_finish: bad sizes (blocks=%d steps=%d sequences=%d)", blocks, steps, n_seq);
    const int64_t n = (int64_t)steps * n_seq;
    if (n == 0) return CVX_OK;
    hipLaunchKernelGGL(rk_err_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cvx_hip_stream(s),
                       reinterpret_cast<const float2*>(partials), map_dev, reinterpret_cast<float2*>(err), steps, n_seq, blocks);
    CVX_CHECK_LAUNCH("cvx_rk_err_finish_f32");
    return CVX_OK;
}

extern "C" int cvx_embed_gather_f32(const int64_t* ids, int32_t S, const float* table, int32_t E, int32_t n_rows_table,
                                    const float* cond, const float* cond_row, int32_t Cc, int64_t null_id,
                                    float* out, int64_t M, cvx_stream_t s)
{
    CVX_REQUIRE(table && out && S > 0 && E > 0 && Cc >= 0 && M >= 0, "embed_gather: bad arguments");
    CVX_REQUIRE(cond || cond_row || Cc == 0, "embed_gather: cond and cond_row both null");
    if (M == 0) return CVX_OK;
    hipLaunchKernelGGL(embed_gather_kernel, dim3((unsigned)M), dim3(256), 0, cvx_hip_stream(s),
                       ids, S, table, E, n_rows_table, cond, cond_row, Cc, null_id, out);
    CVX_CHECK_LAUNCH("cvx_embed_gather_f32");
    return CVX_OK;
}

extern "C" int cvx_time_fourier_f32(const float* times, const float* w, float* out, int32_t n, int32_t half, cvx_stream_t s)
{
    CVX_REQUIRE(times && w && out && n >= 0 && half > 0, "time_fourier: bad arguments");
    if (n == 0) return CVX_OK;
    hipLaunchKernelGGL(time_fourier_kernel, dim3(n), dim3(256), 0, cvx_hip_stream(s), times, w, out, half);
    CVX_CHECK_LAUNCH("cvx_time_fourier_f32");
    return CVX_OK;
}

extern "C" int cvx_wav_to_int16(const float* wav, int16_t* pcm, int64_t n, cvx_stream_t s)
{
    CVX_REQUIRE(wav && pcm && n >= 0, "wav_to_int16: bad arguments");
    if (n == 0) return CVX_OK;
    hipLaunchKernelGGL(wav_to_int16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cvx_hip_stream(s), wav, pcm, n);
    CVX_CHECK_LAUNCH("cvx_wav_to_int16");
    return CVX_OK;
}
