// Dynamic time warping of MANY pairs of feature sequences in one launch (cvx_dtw_f32; include/covomix_hip.h, "DTW"): the cost and the
// length of the best warping path, what the mel-cepstral distortion of the acoustic model is counted with (metrics.py).
//
// One 256-thread block per pair, the pipeline of csrc/edit_distance.hip.  The SHORTER item (m frames) lies on the rows, in BANDS of
// 256 K rows: thread t of a band holds its K consecutive frames in registers (W floats each, dim padded to W = 16, 32 or 80 with zeros;
// K = 4, 4, 1).  The LONGER item (n frames) streams through a RING of 320 columns in LDS, refilled 64 columns at a time: at step s
// thread t works on column s - t, so one step touches columns s - 255 ... s and 255 + 64 <= 320 never overwrites a column still in use.
// A ring row is W + 4 words: neighbouring threads read neighbouring rows with ds_read_b128, and 20 (36, 84) words a row put the 16
// lanes of a read group on 16 different bank quads.  Per step a thread reads one column (W words), computes its K frame distances and K
// cells, and hands ONE (cost, steps) cell to thread t + 1 through two alternating LDS rows; one block barrier per step, n + T - 1 steps
// for a band of T threads.  The last row of a band stays in LDS (8 bytes a column, only sized when some pair of the call has more than
// one band) as the top row of the next band.  The result is cell (m - 1, n - 1): the thread that owns it stores cost and steps, the
// only two stores of the block.  No global scratch, no atomics, no private segment; no frame outside an item and no column behind dim
// is read.
//
// The arithmetic is fixed to the bit (the header states it): every subtraction, product, sum and square root is an individually
// rounded fp32 operation.  They are written as plain operators with contraction OFF for this file, and sqrtf: the __fmul_rn / __fadd_rn
// of the HIP headers are plain operators compiled where contraction is allowed (the compiler fuses them into v_fmac_f32 after
// inlining) and __fsqrt_rn is the bare v_sqrt_f32 (1 ulp); sqrtf is the correctly rounded sequence.  The cells are chosen by a
// lexicographic minimum on (cost, steps), so neither the order of the three comparisons nor which item lies on the rows changes a bit.
#include "cvx_common.h"
#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr int DTW_THREADS = 256;
constexpr int DTW_CHUNK = 64;                         // columns per refill of the ring
constexpr int DTW_RING = 320;                         // columns in LDS: >= DTW_THREADS - 1 + DTW_CHUNK
static_assert(DTW_RING >= DTW_THREADS - 1 + DTW_CHUNK, "a refill must not overwrite a column a thread still reads");

struct DtwCell { float c; int s; };                   // 8 bytes: one ds_read_b64 / ds_write_b64

__device__ __forceinline__ DtwCell dtw_min(DtwCell a, DtwCell b) { return (b.c < a.c || (b.c == a.c && b.s < a.s)) ? b : a; }

// four floats of row `row` from column d on; columns behind dim read as +0 (they may hold anything in memory)
__device__ __forceinline__ float4 dtw_load4(const float* __restrict__ base, int64_t ld, int64_t row, int d, int dim)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d < dim) {                                    // ld % 4 == 0 and ld >= dim: the whole quad lies inside the row
        v = *reinterpret_cast<const float4*>(base + row * ld + d);
        if (d + 1 >= dim) v.y = 0.f;
        if (d + 2 >= dim) v.z = 0.f;
        if (d + 3 >= dim) v.w = 0.f;
    }
    return v;
}

template <int W, int K>
__global__ __launch_bounds__(DTW_THREADS) void dtw_kernel(const float* __restrict__ frames, int64_t n_rows, int64_t ld, int dim,
                                                          const int32_t* __restrict__ items, int n_items,
                                                          const int32_t* __restrict__ pairs, int carry_cols,
                                                          float* __restrict__ cost, int32_t* __restrict__ steps)
{
    constexpr int STRIDE = W + 4;                     // words per ring row
    constexpr int Q = W / 4;
    constexpr int BAND = DTW_THREADS * K;             // rows per band
    extern __shared__ __align__(16) unsigned char dtw_lds[];
    DtwCell* xch = reinterpret_cast<DtwCell*>(dtw_lds);                                   // [2][256] hand-over rows
    float* ring = reinterpret_cast<float*>(dtw_lds + 2 * DTW_THREADS * sizeof(DtwCell));  // [DTW_RING][STRIDE]
    DtwCell* carry = reinterpret_cast<DtwCell*>(ring + DTW_RING * STRIDE);                // [carry_cols]: a band's last row
    const int t = threadIdx.x;
    const int p = blockIdx.x;
    const float INF = __int_as_float(0x7f800000), QNAN = __int_as_float(0x7fc00000);

    // the DEVICE copies of this block's table rows, before any frame is read: rows that break what the entry point checked on the host
    // copies give (NaN, -1)
    const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
    bool bad = ia < 0 || ia >= n_items || ib < 0 || ib >= n_items;
    int64_t oa = 0, ob = 0;
    int la = 0, lb = 0;
    if (!bad) {
        oa = items[2 * ia]; la = items[2 * ia + 1];
        ob = items[2 * ib]; lb = items[2 * ib + 1];
        bad = oa < 0 || ob < 0 || la < 0 || lb < 0 || la > CVX_DTW_MAX_FRAMES || lb > CVX_DTW_MAX_FRAMES || oa + la > n_rows || ob + lb > n_rows ||
              (min(la, lb) > BAND && max(la, lb) > carry_cols);
    }
    if (bad) { if (t == 0) { cost[p] = QNAN; steps[p] = -1; } return; }
    if (la == 0 || lb == 0) { if (t == 0) { cost[p] = 0.f; steps[p] = 0; } return; }
    if (la > lb) { const int64_t o = oa; oa = ob; ob = o; const int l = la; la = lb; lb = l; }      // the rule is symmetric: a is the shorter
    const int m = la, n = lb;

    const int bands = (m + BAND - 1) / BAND;
    for (int band = 0; band < bands; ++band) {
        const int mb = min(m - band * BAND, BAND);    // rows of this band
        const int T = (mb + K - 1) / K;               // threads with a row
        const bool last = band == bands - 1;
        const int r0 = band * BAND + t * K;           // rows r0 ... r0 + K - 1
        float x[K][W];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float4 v = r0 + k < m ? dtw_load4(frames, ld, oa + r0 + k, 4 * q, dim) : make_float4(0.f, 0.f, 0.f, 0.f);
                x[k][4 * q] = v.x; x[k][4 * q + 1] = v.y; x[k][4 * q + 2] = v.z; x[k][4 * q + 3] = v.w;
            }
        DtwCell col[K];                               // this strip's cells of the column to the left: nothing lies left of column 0
#pragma unroll
        for (int k = 0; k < K; ++k) col[k] = DtwCell{INF, 0};
        DtwCell topleft = r0 == 0 ? DtwCell{0.f, 0} : DtwCell{INF, 0};      // the path starts diagonally above cell (0, 0) with no cost and no steps
        int slot = t == 0 ? 0 : DTW_RING - t;         // ring row of column s - t
        const int nsteps = n + T - 1;
        for (int s = 0; s < nsteps; ++s) {
            if (s % DTW_CHUNK == 0) {                 // columns s ... s + 63 enter the ring; the barrier that ended step s - 1 freed their rows
                const int cnt = min(DTW_CHUNK, n - s);
                for (int idx = t; idx < cnt * Q; idx += DTW_THREADS) {
                    const int j = s + idx / Q, q = idx % Q;
                    *reinterpret_cast<float4*>(ring + (j % DTW_RING) * STRIDE + 4 * q) = dtw_load4(frames, ld, ob + j, 4 * q, dim);
                }
                __syncthreads();
            }
            const int j = s - t;                      // this thread's column of the step
            if (t < T && j >= 0 && j < n) {
                DtwCell top;                          // cell (r0 - 1, j): thread t - 1 stored it one step ago; the band above left it; or nothing
                if (t > 0) top = xch[((s - 1) & 1) * DTW_THREADS + t - 1];
                else if (band > 0) top = carry[j];
                else top = DtwCell{INF, 0};
                const float* y = ring + slot * STRIDE;
                float acc[K];
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] = 0.f;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const float4 yv = *reinterpret_cast<const float4*>(y + 4 * q);
                    const float ye[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const float diff = x[k][4 * q + e] - ye[e];
                            acc[k] = acc[k] + diff * diff;
                        }
                }
                DtwCell up = top, diag = topleft;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const DtwCell left = col[k];
                    const DtwCell best = dtw_min(dtw_min(up, left), diag);
                    const DtwCell v = DtwCell{sqrtf(acc[k]) + best.c, best.s + 1};
                    diag = left; up = v; col[k] = v;
                }
                topleft = top;
                if (t + 1 < T) xch[(s & 1) * DTW_THREADS + t] = col[K - 1];
                else if (!last) carry[j] = col[K - 1];          // T = 256 here: the next band's thread 0 reads it
            }
            slot = slot + 1 == DTW_RING ? 0 : slot + 1;
            __syncthreads();                          // step s + 1 reads row s & 1 and overwrites row (s - 1) & 1, which step s read
        }
        if (last && t == T - 1) {                     // cell (m - 1, n - 1) is row (mb - 1) % K of the last strip
            DtwCell res = col[0];
            const int km = (mb - 1) % K;
#pragma unroll
            for (int k = 1; k < K; ++k) if (k == km) res = col[k];
            cost[p] = res.c;
            steps[p] = res.s;
        }
    }
}

template <int W, int K>
int dtw_launch(const float* frames, int64_t n_rows, int64_t ld, int dim, const int32_t* items_host, const int32_t* items_dev, int n_items,
               const int32_t* pairs_host, const int32_t* pairs_dev, int n_pairs, float* cost, int32_t* steps, cvx_stream_t s)
{
    int carry_cols = 0;                               // the longest item of a pair whose shorter item needs more than one band
    for (int p = 0; p < n_pairs; ++p) {
        const int la = items_host[2 * pairs_host[2 * p] + 1], lb = items_host[2 * pairs_host[2 * p + 1] + 1];
        if (std::min(la, lb) > DTW_THREADS * K) carry_cols = std::max(carry_cols, std::max(la, lb));
    }
    carry_cols = (carry_cols + DTW_THREADS - 1) / DTW_THREADS * DTW_THREADS;
    const size_t lds = 2 * DTW_THREADS * sizeof(DtwCell) + (size_t)DTW_RING * (W + 4) * sizeof(float) + (size_t)carry_cols * sizeof(DtwCell);
    cvx_allow_dynamic_lds(reinterpret_cast<const void*>(dtw_kernel<W, K>), (int)lds);   // 29.6 ... 141 KB
    hipLaunchKernelGGL((dtw_kernel<W, K>), dim3((unsigned)n_pairs), dim3(DTW_THREADS), lds, cvx_hip_stream(s), frames, n_rows, ld, dim,
                       items_dev, n_items, pairs_dev, carry_cols, cost, steps);
    CVX_CHECK_LAUNCH("cvx_dtw_f32");
    return CVX_OK;
}

}  // namespace

static_assert(CVX_DTW_MAX_DIM == 80 && CVX_DTW_MAX_DIM % 4 == 0, "the widest instance holds CVX_DTW_MAX_DIM columns");
static_assert(2 * DTW_THREADS * 8 + DTW_RING * (CVX_DTW_MAX_DIM + 4) * 4 + CVX_DTW_MAX_FRAMES * 8 <= 160 * 1024,
              "hand-over rows + ring + carry row of the widest instance fit one block's LDS");

extern "C" int cvx_dtw_f32(const float* frames_dev, int64_t n_rows, int64_t ld, int32_t dim, const int32_t* items_host,
                           const int32_t* items_dev, int32_t n_items, const int32_t* pairs_host, const int32_t* pairs_dev, int32_t n_pairs,
                           float* cost_dev, int32_t* steps_dev, cvx_stream_t s)
{
    CVX_REQUIRE(n_rows >= 0 && n_items >= 0 && n_pairs >= 0, "dtw: negative count (%ld rows, %d items, %d pairs)", (long)n_rows, n_items, n_pairs);
    CVX_REQUIRE(dim >= 1 && dim <= CVX_DTW_MAX_DIM, "dtw: dim = %d (1 ... %d)", dim, CVX_DTW_MAX_DIM);
    CVX_REQUIRE(ld >= dim && ld % 4 == 0, "dtw: ld = %ld for dim = %d (ld >= dim, a multiple of 4)", (long)ld, dim);
    CVX_REQUIRE(reinterpret_cast<uintptr_t>(frames_dev) % 16 == 0, "dtw: the frames are not 16-byte aligned");
    CVX_REQUIRE(n_items == 0 || items_host, "dtw: no host copy of the item table");
    CVX_REQUIRE(n_pairs == 0 || pairs_host, "dtw: no host copy of the pair table");
    for (int32_t i = 0; i < n_items; ++i) {
        const int64_t row = items_host[2 * i], len = items_host[2 * i + 1];
        CVX_REQUIRE(len >= 0 && len <= CVX_DTW_MAX_FRAMES, "dtw: item %d has %ld frames (0 ... %d)", i, (long)len, CVX_DTW_MAX_FRAMES);
        CVX_REQUIRE(row >= 0 && row + len <= n_rows, "dtw: item %d = rows [%ld, %ld) lies outside the %ld rows of the call", i, (long)row,
                    (long)(row + len), (long)n_rows);
    }
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t a = pairs_host[2 * p], b = pairs_host[2 * p + 1];
        CVX_REQUIRE(a >= 0 && a < n_items && b >= 0 && b < n_items, "dtw: pair %d names items (%d, %d) of %d", p, a, b, n_items);
    }
    if (n_pairs == 0) return CVX_OK;
    CVX_REQUIRE(items_dev && pairs_dev && cost_dev && steps_dev && (frames_dev || n_rows == 0), "dtw: null device pointer");
    if (dim <= 16)
        return dtw_launch<16, 4>(frames_dev, n_rows, ld, dim, items_host, items_dev, n_items, pairs_host, pairs_dev, n_pairs, cost_dev, steps_dev, s);
    if (dim <= 32)
        return dtw_launch<32, 4>(frames_dev, n_rows, ld, dim, items_host, items_dev, n_items, pairs_host, pairs_dev, n_pairs, cost_dev, steps_dev, s);
    return dtw_launch<80, 1>(frames_dev, n_rows, ld, dim, items_host, items_dev, n_items, pairs_host, pairs_dev, n_pairs, cost_dev, steps_dev, s);
}
