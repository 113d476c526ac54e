// Unit-cost Levenshtein distance of MANY pairs of token sequences in one launch (cvx_edit_distance_i64; include/covomix_hip.h, "EDIT
// DISTANCE"): what consensus best-of-N (t2s.consensus_risks) and the token error rate (t2s.token_error_rate) are counted with.
//
// One 256-thread block per pair.  The SHORTER item of the pair (m tokens) lies in registers: thread t owns the K consecutive rows
// t K + 1 ... t K + K of the DP matrix, K = 1, 2, 4, 8 or 16 by m (m <= 256 K), and keeps its K cells of the column it finished last.
// The LONGER item (n tokens) is staged in LDS, narrowed to int32.  The threads run as a pipeline over the columns: at step s thread
// t computes column s - t + 1 of its strip - K cells, each from the cell above it (a register, or for the strip's first row the bottom
// cell thread t - 1 stored one step earlier), the cell to its left and the cell diagonally above (registers).  What crosses a thread
// is ONE word per step, through two alternating rows of LDS, with one block barrier per step: n + ceil(m / K) - 1 steps for the pair,
// not the m + n of an anti-diagonal sweep, and per cell no LDS access at all (the anti-diagonal layout reads three diagonals and both
// tokens per cell).  LDS: 4 n_max bytes for the longer item (at most 16 KB) + 2 KB for the hand-over rows; several blocks share a CU.
// The distance is cell (m, n): the last cell of thread ceil(m / K) - 1's strip after the last step - that thread stores it, the only
// store of the block.  int32 throughout; no global scratch, no atomics; no token behind an item's length is read.
#include "cvx_common.h"
#include <algorithm>

namespace {

constexpr int ED_THREADS = 256;

// The pair with its shorter item (ta, m >= 1 tokens) on strips of K rows a thread; sb = the longer item in LDS.  Stores the distance.
template <int K>
__device__ __forceinline__ void ed_strip(const int64_t* __restrict__ ta, int m, const int32_t* sb, int n, int32_t* xch, int32_t* out)
{
    const int t = threadIdx.x;
    const int T = (m + K - 1) / K;                    // threads with a row
    const int r0 = t * K;                             // rows r0 + 1 ... r0 + K (1-based), tokens ta[r0 ... r0 + K - 1]
    int32_t a[K], col[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        a[k] = r0 + k < m ? (int32_t)ta[r0 + k] : 0;  // rows behind m: computed, never looked at
        col[k] = r0 + k + 1;                          // column 0: D[i][0] = i
    }
    int topleft = r0;                                 // D[r0][0]
    const int steps = n + T - 1;
    for (int s = 0; s < steps; ++s) {
        const int j = s - t + 1;                      // this thread's column of the step
        if (t < T && j >= 1 && j <= n) {
            const int32_t bj = sb[j - 1];
            const int top = t == 0 ? j : xch[((s - 1) & 1) * ED_THREADS + t - 1];       // D[r0][j]: thread t - 1 stored it at step s - 1
            int diag = topleft, up = top;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int left = col[k];
                const int v = min(min(left, up) + 1, diag + (a[k] != bj ? 1 : 0));
                diag = left; up = v; col[k] = v;
            }
            topleft = top;
            xch[(s & 1) * ED_THREADS + t] = col[K - 1];
        }
        __syncthreads();                              // step s + 1 reads row s & 1 and overwrites row (s - 1) & 1, which step s read
    }
    if (t != T - 1) return;                           // cell (m, n) is row (m - 1) % K of the last strip
    int res = 0;
    const int km = (m - 1) % K;
#pragma unroll
    for (int k = 0; k < K; ++k) if (k == km) res = col[k];
    *out = res;
}

// A block looks at the DEVICE copies of its table rows before it reads a token: rows that break what the entry point checked on the
// host copies (the caller uploaded something else) give -1 and read nothing.
__global__ __launch_bounds__(ED_THREADS) void edit_distance_kernel(const int64_t* __restrict__ tokens, int64_t n_tokens,
                                                                   const int32_t* __restrict__ items, int n_items,
                                                                   const int32_t* __restrict__ pairs, int lds_tokens,
                                                                   int32_t* __restrict__ out)
{
    extern __shared__ int32_t ed_lds[];               // [2][256] hand-over rows, then the longer item
    int32_t* xch = ed_lds;
    int32_t* sb = ed_lds + 2 * ED_THREADS;
    const int p = blockIdx.x;
    const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
    if (ia < 0 || ia >= n_items || ib < 0 || ib >= n_items) { if (threadIdx.x == 0) out[p] = -1; return; }
    int64_t oa = items[2 * ia], ob = items[2 * ib];
    int la = items[2 * ia + 1], lb = items[2 * ib + 1];
    if (oa < 0 || ob < 0 || la < 0 || lb < 0 || la > CVX_EDIT_MAX_LEN || lb > CVX_EDIT_MAX_LEN || oa + la > n_tokens || ob + lb > n_tokens ||
        max(la, lb) > lds_tokens) {
        if (threadIdx.x == 0) out[p] = -1;
        return;
    }
    if (la > lb) { const int64_t o = oa; oa = ob; ob = o; const int l = la; la = lb; lb = l; }      // the distance is symmetric: a is the shorter
    const int m = la, n = lb;
    if (m == 0) { if (threadIdx.x == 0) out[p] = n; return; }
    const int64_t* tb = tokens + ob;
    for (int j = threadIdx.x; j < n; j += ED_THREADS) sb[j] = (int32_t)tb[j];
    __syncthreads();
    const int64_t* ta = tokens + oa;
    if (m <= ED_THREADS) ed_strip<1>(ta, m, sb, n, xch, out + p);
    else if (m <= 2 * ED_THREADS) ed_strip<2>(ta, m, sb, n, xch, out + p);
    else if (m <= 4 * ED_THREADS) ed_strip<4>(ta, m, sb, n, xch, out + p);
    else if (m <= 8 * ED_THREADS) ed_strip<8>(ta, m, sb, n, xch, out + p);
    else ed_strip<16>(ta, m, sb, n, xch, out + p);
}

}  // namespace

static_assert(CVX_EDIT_MAX_LEN == 16 * ED_THREADS, "the widest strip (16 rows a thread) holds the longest item");

extern "C" int cvx_edit_distance_i64(const int64_t* tokens_dev, int64_t n_tokens, const int32_t* items_host, const int32_t* items_dev,
                                     int32_t n_items, const int32_t* pairs_host, const int32_t* pairs_dev, int32_t n_pairs, int32_t* out_dev,
                                     cvx_stream_t s)
{
    CVX_REQUIRE(n_tokens >= 0 && n_items >= 0 && n_pairs >= 0, "edit_distance: negative count (%ld tokens, %d items, %d pairs)",
                (long)n_tokens, n_items, n_pairs);
    CVX_REQUIRE(n_items == 0 || items_host, "edit_distance: no host copy of the item table");
    CVX_REQUIRE(n_pairs == 0 || pairs_host, "edit_distance: no host copy of the pair table");
    for (int32_t i = 0; i < n_items; ++i) {
        const int64_t off = items_host[2 * i], len = items_host[2 * i + 1];
        CVX_REQUIRE(len >= 0 && len <= CVX_EDIT_MAX_LEN, "edit_distance: item %d has length %ld (0 ... %d)", i, (long)len, CVX_EDIT_MAX_LEN);
        CVX_REQUIRE(off >= 0 && off + len <= n_tokens, "edit_distance: item %d = tokens [%ld, %ld) lies outside the %ld tokens of the call",
                    i, (long)off, (long)(off + len), (long)n_tokens);
    }
    int longest = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t a = pairs_host[2 * p], b = pairs_host[2 * p + 1];
        CVX_REQUIRE(a >= 0 && a < n_items && b >= 0 && b < n_items, "edit_distance: pair %d names items (%d, %d) of %d", p, a, b, n_items);
        longest = std::max(longest, std::max(items_host[2 * a + 1], items_host[2 * b + 1]));
    }
    if (n_pairs == 0) return CVX_OK;
    CVX_REQUIRE(items_dev && pairs_dev && out_dev && (tokens_dev || n_tokens == 0), "edit_distance: null device pointer");
    const int lds_tokens = (longest + ED_THREADS - 1) / ED_THREADS * ED_THREADS;
    const size_t lds = (size_t)(2 * ED_THREADS + lds_tokens) * sizeof(int32_t);          // at most 18 KB
    hipLaunchKernelGGL(edit_distance_kernel, dim3((unsigned)n_pairs), dim3(ED_THREADS), lds, cvx_hip_stream(s), tokens_dev, n_tokens,
                       items_dev, n_items, pairs_dev, lds_tokens, out_dev);
    CVX_CHECK_LAUNCH("cvx_edit_distance_i64");
    return CVX_OK;
}
