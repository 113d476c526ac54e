// The row-local kernels of one network evaluation with a TIME PER SEQUENCE of a packed batch (gfx950), and of the
// conditional-flow-matching loss that sits on it (reference acoustic.py:732-791 on CoVoMix.forward(..., target=flow), :430-538):
//   cvx_adarmsnorm_seq_f32     AdaptiveRMSNorm with one gamma / beta row per sequence (cu_seqlens)
//   cvx_cfm_inputs_f32         w = (1 - (1 - sigma) t) x0 + t x1, flow = x1 - (1 - sigma) x0, cond with its masked rows zeroed
//   cvx_masked_mse_f32         per row mean_d (pred - flow)^2, per sequence the masked mean of those
// All of them stream rows once: one wavefront per row, no LDS beyond the block reduction of the loss, no scratch, no atomics
// besides the saturation commit every split-pair producer carries.  A row's sequence is found by a wave-uniform binary search
// over cu (at most 12 steps of scalar loads from a table of <= 16 KB that stays in the scalar cache).  The HOST copy of cu is
// validated before anything is launched and sizes the launch; the kernels take their row range from it and use the DEVICE copy
// only to pick a sequence index, which the search keeps inside [0, n_seq) whatever that copy holds.
#include "cvx_common.h"

namespace {

__device__ __forceinline__ float seq_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

typedef _Float16 seq_f16x4 __attribute__((ext_vector_type(4)));
// split 4 floats into fp16 (hi, lo) and store 8 bytes each: the plain and the interleaved (lo == hi + 32) pair layouts of
// elementwise.hip's store_split4, whose arithmetic this repeats operation for operation
__device__ __forceinline__ void seq_store_split4(_Float16* hi, _Float16* lo, int64_t off, const f32x4 o, CvxSat& amax)
{
    cvx_amax4(amax, o);
    if (lo == hi + 32) off = ((off >> 5) << 6) | (off & 31);
    seq_f16x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x = fminf(fmaxf(o[e], -65504.f), 65504.f);
        h[e] = (_Float16)x;
        l[e] = (_Float16)(x - (float)h[e]);
    }
    *reinterpret_cast<seq_f16x4*>(hi + off) = h;
    if (lo) *reinterpret_cast<seq_f16x4*>(lo + off) = l;
}

// the sequence of a row: the largest s in [0, n_seq) with cu[s] <= row for cu[0] <= row < cu[n_seq] (sequences without rows are
// stepped over).  Reads cu[1 .. n_seq - 1] only; the result is inside [0, n_seq) for ANY table contents.  `row` is wave-uniform.
__device__ __forceinline__ int seq_of_row(const int32_t* __restrict__ cu, int n_seq, int row)
{
    int lo = 0, hi = n_seq - 1;                  // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;      // in [1, n_seq - 1]
        if (cu[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------- AdaRMSNorm, gamma / beta row per sequence
// adarmsnorm_kernel<NV> of elementwise.hip with `g = row / rows_per_group` replaced by the search and the group rows
// `group_stride` floats apart; every arithmetic statement is that kernel's, in its order.
template <int NV>
__global__ __launch_bounds__(256) void adanorm_seq_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ y,
                                                         _Float16* __restrict__ y_hi, _Float16* __restrict__ y_lo,
                                                         int row0, int row_end, int D, const int32_t* __restrict__ cu, int n_seq,
                                                         int64_t group_stride, float scale, float eps,
                                                         const float* __restrict__ split_scale, uint32_t* __restrict__ sat)
{
    const int lane = threadIdx.x & 63;
    const int wrow = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t row = (int64_t)row0 + (int64_t)blockIdx.x * 4 + wrow;
    if (row >= row_end) return;
    CvxSat amax;
    const float ssc = split_scale ? *split_scale : 1.f;
    const float* xr = x + row * D;
    const int64_t g = seq_of_row(cu, n_seq, (int)row);
    const float* gr = gamma + g * group_stride;
    const float* br = beta ? beta + g * group_stride : nullptr;
    float* yr = y ? y + row * D : nullptr;
    const int nvec = D >> 2;

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
    ss = seq_wave_sum(ss);
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
            if (y_hi) { const f32x4 os = {o[0] * ssc, o[1] * ssc, o[2] * ssc, o[3] * ssc}; seq_store_split4(y_hi, y_lo, row * D + 4 * j, os, amax); }
        }
    }
    cvx_sat_commit(sat, amax);
}

// generic-D fallback: two passes over the row (adarmsnorm_generic_kernel)
__global__ __launch_bounds__(256) void adanorm_seq_generic_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float* __restrict__ y,
                                                                 _Float16* __restrict__ y_hi, _Float16* __restrict__ y_lo,
                                                                 int row0, int row_end, int D, const int32_t* __restrict__ cu, int n_seq,
                                                                 int64_t group_stride, float scale, float eps,
                                                                 const float* __restrict__ split_scale, uint32_t* __restrict__ sat)
{
    const int lane = threadIdx.x & 63;
    const int wrow = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t row = (int64_t)row0 + (int64_t)blockIdx.x * 4 + wrow;
    if (row >= row_end) return;
    CvxSat amax;
    const float ssc = split_scale ? *split_scale : 1.f;
    const float* xr = x + row * D;
    const int64_t g = seq_of_row(cu, n_seq, (int)row);
    float ss = 0.f;
    for (int j = lane; j < (D >> 2); j += 64) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xr + 4 * j);
        ss += t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3];
    }
    ss = seq_wave_sum(ss);
    const float inv = scale / fmaxf(sqrtf(ss), eps);
    for (int j = lane; j < (D >> 2); j += 64) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xr + 4 * j);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(gamma + g * group_stride + 4 * j);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = t[e] * inv * gg[e];
        if (beta) {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(beta + g * group_stride + 4 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += bb[e];
        }
        if (y) *reinterpret_cast<f32x4*>(y + row * D + 4 * j) = o;
        if (y_hi) { const f32x4 os = {o[0] * ssc, o[1] * ssc, o[2] * ssc, o[3] * ssc}; seq_store_split4(y_hi, y_lo, row * D + 4 * j, os, amax); }
    }
    cvx_sat_commit(sat, amax);
}

// From here to the end of the file NO implicit a * b + c -> fma contraction: the kernels below promise individually rounded
// operations (a numpy restatement is compared with ==), and the __fmul_rn / __fadd_rn of the HIP headers are plain operators the
// compiler fuses after inlining.  The norm kernels above stay under the default, as the kernel they repeat is.
#pragma clang fp contract(off)

// ---------------------------------------------------------------- the inputs of the loss evaluation
// one wavefront per row; a lane owns 16-byte pieces of the row: [0, dv) of x0 / x1 -> w, flow, [dv, dv + cv) of cond -> cond_in.
// Every operation is an individually rounded fp32 operation (contraction is off), in the order the header states.
__global__ __launch_bounds__(256) void cfm_inputs_kernel(const float* __restrict__ x1, const float* __restrict__ x0,
                                                        const float* __restrict__ cond, const uint8_t* __restrict__ mask,
                                                        const float* __restrict__ times, const int32_t* __restrict__ cu, int n_seq,
                                                        int row0, int row_end, int dv, int cv, float sigma,
                                                        float* __restrict__ w, float* __restrict__ flow, float* __restrict__ cond_in)
{
    const int lane = threadIdx.x & 63;
    const int wrow = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t row = (int64_t)row0 + (int64_t)blockIdx.x * 4 + wrow;
    if (row >= row_end) return;
    const int s = seq_of_row(cu, n_seq, (int)row);
    const float t = times[s];
    const bool masked = mask[row] != 0;
    const float oms = 1.f - sigma;                            // 1 - sigma
    const float c0 = 1.f - oms * t;                    // 1 - (1 - sigma) t
    for (int j = lane; j < dv + cv; j += 64) {
        if (j < dv) {
            const int64_t off = row * (4 * (int64_t)dv) + 4 * j;
            const f32x4 a1 = gload4(x1 + off), a0 = gload4(x0 + off);
            f32x4 ow, of;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ow[e] = c0 * a0[e] + t * a1[e];
                of[e] = a1[e] - oms * a0[e];
            }
            *reinterpret_cast<f32x4*>(w + off) = ow;
            *reinterpret_cast<f32x4*>(flow + off) = of;
        } else {
            const int64_t off = row * (4 * (int64_t)cv) + 4 * (j - dv);
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            if (!masked) c = gload4(cond + off);
            *reinterpret_cast<f32x4*>(cond_in + off) = c;
        }
    }
}

// ---------------------------------------------------------------- the masked loss
// stage 1: e[r] = (sum_d (pred[r, d] - flow[r, d])^2) / dim.  One wavefront per row; lane l sums d = l, l + 64, ... in that order
// starting from +0 (a coalesced request of whole lines per 64 columns), then the 6 levels of the xor butterfly (32, 16, .. 1).
// Every operation individually rounded: ceil(dim / 64) + 6 additions above a term.
__global__ __launch_bounds__(256) void cfm_row_mse_kernel(const float* __restrict__ pred, const float* __restrict__ flow, int row0, int row_end,
                                                         int dim, float* __restrict__ err_rows)
{
    const int lane = threadIdx.x & 63;
    const int wrow = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t row = (int64_t)row0 + (int64_t)blockIdx.x * 4 + wrow;
    if (row >= row_end) return;
    const float* p = pred + row * dim;
    const float* f = flow + row * dim;
    float acc = 0.f;
    for (int d = lane; d < dim; d += 64) {
        const float df = p[d] - f[d];
        acc = acc + df * df;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
    if (lane == 0) err_rows[row] = acc / (float)dim;
}

// stage 2: one block per sequence.  Thread t sums the masked e of the sequence's rows t, t + 256, ... (counted from the sequence's
// own first row) in that order from +0, the wave butterfly (6 levels) follows, then the four wave sums as (w0 + w1) + (w2 + w3):
// ceil(T / 256) + 8 additions above a term - CVX_MASKED_MSE_TREE_DEPTH(T) - and nothing depends on where the sequence sits.
__global__ __launch_bounds__(256) void cfm_seq_loss_kernel(const float* __restrict__ err_rows, const uint8_t* __restrict__ mask,
                                                          const int32_t* __restrict__ cu, int n_seq, int row_lo, int row_hi,
                                                          float* __restrict__ loss, int32_t* __restrict__ count)
{
    __shared__ float s_num[4];
    __shared__ int s_cnt[4];
    const int s = blockIdx.x;
    // the DEVICE offsets, clamped into the row range the host validated: a table that differs from the host copy reads no row outside it
    const int r0 = min(max(cu[s], row_lo), row_hi), r1 = min(max(cu[s + 1], r0), row_hi);
    float acc = 0.f;
    int cnt = 0;
    for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) {
        const bool m = mask[r] != 0;
        acc = acc + (m ? err_rows[r] : 0.f);
        cnt += m ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc = acc + __shfl_xor(acc, o, 64);
        cnt += __shfl_xor(cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_num[threadIdx.x >> 6] = acc; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float num = (s_num[0] + s_num[1]) + (s_num[2] + s_num[3]);
        const int c = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        loss[s] = num / fmaxf((float)c, 1e-5f);                  // mask.sum().clamp(min = 1e-5), acoustic.py:535
        count[s] = c;
    }
}

// the host copy of cu: n_seq + 1 non-decreasing offsets inside [0, rows]
bool cu_ok(const int32_t* cu, int32_t n_seq, int64_t rows)
{
    if (cu[0] < 0) return false;
    for (int32_t i = 0; i < n_seq; ++i)
        if (cu[i + 1] < cu[i]) return false;
    return (int64_t)cu[n_seq] <= rows;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int cvx_adarmsnorm_seq_f32(const float* x, const float* gamma, const float* beta, float* y, uint16_t* y_hi_, uint16_t* y_lo_,
                                      int64_t rows, int32_t D, const int32_t* cu_host, const int32_t* cu_dev, int32_t n_seq,
                                      int64_t group_stride, float scale, float eps, const float* split_scale_dev, cvx_stream_t s)
{
    CVX_REQUIRE(x && gamma && (y || y_hi_) && (y_hi_ || !y_lo_), "adarmsnorm_seq: null pointer");
    _Float16* y_hi = reinterpret_cast<_Float16*>(y_hi_);
    _Float16* y_lo = reinterpret_cast<_Float16*>(y_lo_);
    CVX_REQUIRE(rows >= 0 && rows < ((int64_t)1 << 31) && D > 0 && D % 4 == 0, "adarmsnorm_seq: bad shape rows=%ld D=%d", (long)rows, D);
    CVX_REQUIRE(!(y_hi && y_lo == y_hi + 32) || D % 32 == 0, "adarmsnorm_seq: an interleaved pair (y_lo == y_hi + 32) needs D %% 32 == 0 (D=%d)", D);
    CVX_REQUIRE(cu_host && cu_dev && n_seq >= 1 && n_seq <= CVX_SEQ_NORM_MAX_SEQS, "adarmsnorm_seq: n_seq=%d (1 ... %d) with both copies of cu",
                n_seq, CVX_SEQ_NORM_MAX_SEQS);
    CVX_REQUIRE(group_stride >= D && group_stride % 4 == 0, "adarmsnorm_seq: group_stride=%ld (>= D=%d, a multiple of 4)", (long)group_stride, D);
    CVX_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(y), "adarmsnorm_seq: x, gamma, beta and y must be 16-byte aligned");
    CVX_REQUIRE(cu_ok(cu_host, n_seq, rows), "adarmsnorm_seq: cu must hold %d non-decreasing offsets inside [0, rows=%ld]", n_seq + 1, (long)rows);
    if (y_hi) CVX_REQUIRE_SAT(s);
    const int row0 = cu_host[0], row_end = cu_host[n_seq];
    if (row_end == row0) return CVX_OK;
    hipStream_t st = cvx_hip_stream(s);
    dim3 grid((unsigned)((row_end - row0 + 3) / 4));
    uint32_t* sat = y_hi ? cvx_sat_flag_for(s) : nullptr;
#define SEQ_NORM_ARGS x, gamma, beta, y, y_hi, y_lo, row0, row_end, D, cu_dev, n_seq, group_stride, scale, eps, split_scale_dev, sat
    if (D <= 256)       hipLaunchKernelGGL(adanorm_seq_kernel<1>, grid, dim3(256), 0, st, SEQ_NORM_ARGS);
    else if (D <= 512)  hipLaunchKernelGGL(adanorm_seq_kernel<2>, grid, dim3(256), 0, st, SEQ_NORM_ARGS);
    else if (D <= 1024) hipLaunchKernelGGL(adanorm_seq_kernel<4>, grid, dim3(256), 0, st, SEQ_NORM_ARGS);
    else                hipLaunchKernelGGL(adanorm_seq_generic_kernel, grid, dim3(256), 0, st, SEQ_NORM_ARGS);
#undef SEQ_NORM_ARGS
    CVX_CHECK_LAUNCH("cvx_adarmsnorm_seq_f32");
    return CVX_OK;
}

extern "C" int cvx_cfm_inputs_f32(const float* x1, const float* x0, const float* cond, const uint8_t* mask, const float* times_dev,
                                  const int32_t* cu_host, const int32_t* cu_dev, int32_t n_seq, int64_t rows, int32_t dim_out, int32_t dim_cond,
                                  float sigma, float* w, float* flow, float* cond_in, cvx_stream_t s)
{
    CVX_REQUIRE(x1 && x0 && cond && mask && times_dev && w && flow && cond_in, "cfm_inputs: null pointer");
    CVX_REQUIRE(rows >= 0 && rows < ((int64_t)1 << 31) && dim_out > 0 && dim_out % 4 == 0 && dim_cond > 0 && dim_cond % 4 == 0,
                "cfm_inputs: bad shape rows=%ld dim_out=%d dim_cond=%d (widths: positive multiples of 4)", (long)rows, dim_out, dim_cond);
    CVX_REQUIRE(cu_host && cu_dev && n_seq >= 1 && n_seq <= CVX_SEQ_NORM_MAX_SEQS, "cfm_inputs: n_seq=%d (1 ... %d) with both copies of cu",
                n_seq, CVX_SEQ_NORM_MAX_SEQS);
    CVX_REQUIRE(aligned16(x1) && aligned16(x0) && aligned16(cond) && aligned16(w) && aligned16(flow) && aligned16(cond_in),
                "cfm_inputs: x1, x0, cond, w, flow and cond_in must be 16-byte aligned");
    CVX_REQUIRE(sigma >= 0.f && sigma <= 1.f, "cfm_inputs: sigma=%g outside [0, 1]", (double)sigma);
    CVX_REQUIRE(cu_ok(cu_host, n_seq, rows), "cfm_inputs: cu must hold %d non-decreasing offsets inside [0, rows=%ld]", n_seq + 1, (long)rows);
    const int row0 = cu_host[0], row_end = cu_host[n_seq];
    if (row_end == row0) return CVX_OK;
    hipLaunchKernelGGL(cfm_inputs_kernel, dim3((unsigned)((row_end - row0 + 3) / 4)), dim3(256), 0, cvx_hip_stream(s), x1, x0, cond, mask, times_dev,
                       cu_dev, n_seq, row0, row_end, dim_out / 4, dim_cond / 4, sigma, w, flow, cond_in);
    CVX_CHECK_LAUNCH("cvx_cfm_inputs_f32");
    return CVX_OK;
}

extern "C" int cvx_masked_mse_f32(const float* pred, const float* flow, const uint8_t* mask, const int32_t* cu_host, const int32_t* cu_dev,
                                  int32_t n_seq, int64_t rows, int32_t dim_out, float* err_rows, float* loss, int32_t* count, cvx_stream_t s)
{
    CVX_REQUIRE(pred && flow && mask && err_rows && loss && count, "masked_mse: null pointer");
    CVX_REQUIRE(rows >= 0 && rows < ((int64_t)1 << 31) && dim_out > 0, "masked_mse: bad shape rows=%ld dim_out=%d", (long)rows, dim_out);
    CVX_REQUIRE(cu_host && cu_dev && n_seq >= 1 && n_seq <= CVX_SEQ_NORM_MAX_SEQS, "masked_mse: n_seq=%d (1 ... %d) with both copies of cu",
                n_seq, CVX_SEQ_NORM_MAX_SEQS);
    CVX_REQUIRE(cu_ok(cu_host, n_seq, rows), "masked_mse: cu must hold %d non-decreasing offsets inside [0, rows=%ld]", n_seq + 1, (long)rows);
    const int row0 = cu_host[0], row_end = cu_host[n_seq];
    hipStream_t st = cvx_hip_stream(s);
    if (row_end > row0) {
        hipLaunchKernelGGL(cfm_row_mse_kernel, dim3((unsigned)((row_end - row0 + 3) / 4)), dim3(256), 0, st, pred, flow, row0, row_end, dim_out, err_rows);
        CVX_CHECK_LAUNCH("cvx_masked_mse_f32 (rows)");
    }
    hipLaunchKernelGGL(cfm_seq_loss_kernel, dim3((unsigned)n_seq), dim3(256), 0, st, err_rows, mask, cu_dev, n_seq, row0, row_end, loss, count);
    CVX_CHECK_LAUNCH("cvx_masked_mse_f32");
    return CVX_OK;
}
