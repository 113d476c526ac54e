// text2semantic PREFILL: the attention of one causal full-sequence pass over tokens that are already known (gfx950,
// v_mfma_f32_32x32x2_f32).  The definition: include/covomix_hip.h, cvx_t2s_prefill_attention_f32.
//
// The decode (t2s_decode.hip) spends one step - a chain of dependent launches - on every token, also on the tokens of a forced
// dialogue or a forced prefix, which are all known beforehand.  Their logits come from ONE pass of the target transformer over
// the packed rows of all sequences (t2s.py: _prefill): the row-local parts run on the full-sequence kernels the encoder uses
// (fp32 GEMM with the RoPE epilogue, RMSNorm, GEGLU) and the two attentions of a decoder layer run here:
//   causal  self-attention over the pass' own packed q | k | v rows: the row at position p sees the keys 0..p of its sequence;
//   cross   attention over the decode's context records kv_c = [learned null row | to_kv(encoder)], rows [0, ctx) of a record.
// One kernel carries both: query row r of sequence i, p = r - cu[i], attends to the key rows kbase[i] + j, j < (causal ? p + 1 : nk[i]).
//
// Tiling and the swapped S^T product are those of attention_f32.hip: block = 4 waves = 128 queries of one (sequence, head), a wave
// owns 32 queries; K/V tiles of 32 keys go global -> VGPR -> LDS, double buffered, one barrier per tile; S^T = K . Q^T puts a
// query's scores into one lane pair, O^T += V^T . P^T takes P straight from the accumulator registers.  What differs:
//   * a key is SELECTED by its index (key < the query's count), never masked by adding a large number: rows past a sequence's
//     key count are not even loaded (the tile holds zeros there), so they may hold anything, NaN included;
//   * causal: a block stops at the tile that holds its last query's diagonal, and a wave skips the product of every tile that
//     lies wholly above its own 32 queries (it still helps to stage it);
//   * a block never mixes sequences: blocks are laid out per (sequence, head) for the longest sequence, the others return.
#include "cvx_common.h"

namespace {

constexpr int HD = 64;          // head dim
constexpr int QB = 128;         // queries per block
constexpr int KT = 32;          // keys per tile
constexpr int K_LD = HD + 4;    // padded K row in LDS (floats): conflict-free ds_read_b128
constexpr int V_LD = HD;

struct PrefillAttn {
    const float *q, *k, *v;
    float* out;
    const int32_t *cu, *kbase, *nk;
    int64_t ldq, ldkv;
    int H, n_groups, n_qt, causal;
    float scale_log2e;
};

__global__ __launch_bounds__(256, 2) void t2s_prefill_attention_kernel(const PrefillAttn a)
{
    __shared__ __attribute__((aligned(16))) float Ks[2][KT * K_LD];
    __shared__ __attribute__((aligned(16))) float Vs[2][KT * V_LD];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    // block -> ((sequence, head) group, query tile): the query tiles of one group share blockIdx % 8, i.e. one XCD and one L2
    const int grp = (blockIdx.x / (8 * a.n_qt)) * 8 + (blockIdx.x & 7);
    if (grp >= a.n_groups) return;
    const int head = grp % a.H, seq = grp / a.H;
    const int q_blk = ((blockIdx.x >> 3) % a.n_qt) * QB;
    const int64_t row0 = a.cu[seq];
    const int Lq = a.cu[seq + 1] - (int)row0;
    if (q_blk >= Lq) return;                                    // block-uniform: the grid is sized for the longest sequence
    // keys this block reads: causal - up to its last query's diagonal; cross - the sequence's count
    const int n_keys = a.causal ? min(Lq, q_blk + QB) : max(a.nk[seq], 0);
    const float* qbase = a.q + row0 * a.ldq + head * HD;
    const float* kbase = a.k + (int64_t)a.kbase[seq] * a.ldkv + head * HD;
    const float* vbase = a.v + (int64_t)a.kbase[seq] * a.ldkv + head * HD;

    // ---- Q fragment (B operand of S^T): lane (q = l31, half) holds d = 8c + 4*half + e
    int qrow = q_blk + wid * 32 + l31;
    const bool q_valid = qrow < Lq;
    if (!q_valid) qrow = Lq - 1;
    const int q_count = a.causal ? qrow + 1 : n_keys;          // keys this lane's query sees
    const int w_last = min(q_blk + wid * 32 + 31, Lq - 1);     // the wave's last query (wave-uniform)
    f32x4 qf[8];
#pragma unroll
    for (int c = 0; c < 8; ++c)
        qf[c] = *reinterpret_cast<const f32x4*>(qbase + (int64_t)qrow * a.ldq + 8 * c + 4 * half);

    // ---- staging: a K/V tile is 32 rows x 64 floats = 512 float4 each -> 2 + 2 per thread
    const int s_row = tid >> 4;           // 0..15 (+16 for the second pass)
    const int s_col = (tid & 15) * 4;     // 0..60
    f32x4 rk[2], rv[2];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto load_tile = [&](int key0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = key0 + s_row + 16 * i;
            if (key < n_keys) {
                rk[i] = *reinterpret_cast<const f32x4*>(kbase + (int64_t)key * a.ldkv + s_col);
                rv[i] = *reinterpret_cast<const f32x4*>(vbase + (int64_t)key * a.ldkv + s_col);
            } else { rk[i] = zero4; rv[i] = zero4; }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<f32x4*>(&Ks[buf][(s_row + 16 * i) * K_LD + s_col]) = rk[i];
            *reinterpret_cast<f32x4*>(&Vs[buf][(s_row + 16 * i) * V_LD + s_col]) = rv[i];
        }
    };

    f32x16 o0, o1;                 // O^T tiles: d in [0,32) and [32,64); column = this lane's query
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float m_run = -1e30f;          // running max (in the log2 domain, i.e. of s*scale*log2e)
    float l_run = 0.f;             // this lane's partial of the running denominator

    const int ntiles = (n_keys + KT - 1) / KT;
    load_tile(0);
    store_tile(0);
    __syncthreads();

    for (int it = 0; it < ntiles; ++it) {
        const int cur = it & 1;
        const int key0 = it * KT;
        if (it + 1 < ntiles) load_tile(key0 + KT);

        if (!a.causal || key0 <= w_last) {      // wave-uniform: a tile wholly above the wave's diagonal adds exactly nothing
            // ---- S^T = K . Q^T
            f32x16 sacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
            const float* kp = &Ks[cur][l31 * K_LD + 4 * half];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(kp + 8 * c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], qf[c][e], sacc, 0, 0, 0);
            }

            // ---- online softmax over this lane's 16 keys (+ partner lane's 16); a key past the query's count is not selected
            float mx = -1e30f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = key0 + mfma32_row(r, lane);
                const float sv = (key < q_count) ? sacc[r] * a.scale_log2e : -1e30f;
                sacc[r] = sv;
                mx = fmaxf(mx, sv);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = exp2f(m_run - m_new);
            m_run = m_new;
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = key0 + mfma32_row(r, lane);
                const float pv = (key < q_count) ? exp2f(sacc[r] - m_new) : 0.f;
                sacc[r] = pv;
                psum += pv;
            }
            l_run = l_run * alpha + psum;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }

            // ---- O^T += V^T . P^T   (k pair of MFMA r: keys mfma32_row(r, lane) for the two halves)
            const float* vp = &Vs[cur][l31];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int krow = (r & 3) + 8 * (r >> 2) + 4 * half;
                const float v0 = vp[krow * V_LD];
                const float v1 = vp[krow * V_LD + 32];
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, sacc[r], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, sacc[r], o1, 0, 0, 0);
            }
        }

        if (it + 1 < ntiles) store_tile(cur ^ 1);
        __syncthreads();
    }

    // ---- normalise and store: lane holds O[q][d] for d = dt*32 + (r&3) + 8*(r>>2) + 4*half
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;        // (a sequence without keys, nk <= 0: zeros)
    if (q_valid) {
        const int64_t o_off = (row0 + qrow) * ((int64_t)a.H * HD) + head * HD + 4 * half;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 x, y;
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[e] = o0[4 * g + e] * inv; y[e] = o1[4 * g + e] * inv; }
            *reinterpret_cast<f32x4*>(a.out + o_off + 8 * g) = x;
            *reinterpret_cast<f32x4*>(a.out + o_off + 32 + 8 * g) = y;
        }
    }
}

// rows [0, rows) of a logits buffer [*, width]: l[r] = n + (l[r] - n) * scale[r] with n = l[null_row[r]], the decode's operation order
// (sample_select in t2s_decode.hip: no contraction); a row with null_row[r] < 0 is left alone.  The null rows lie behind `rows`.
__global__ __launch_bounds__(256) void t2s_prefill_guidance_kernel(float* __restrict__ logits, const int32_t* __restrict__ null_row,
                                                                   const float* __restrict__ scale, int64_t rows, int width)
{
    const int64_t r = blockIdx.x;
    const int nr = null_row[r];
    if (nr < 0) return;
    const float s = scale[r];
    float* l = logits + r * width;
    const float* n = logits + (int64_t)nr * width;
    for (int i = threadIdx.x; i < width; i += blockDim.x) {
        const float nv = n[i];
        const float d = __fmul_rn(l[i] - nv, s);
        l[i] = __fadd_rn(nv, d);
    }
}

}  // namespace

extern "C" int cvx_t2s_prefill_attention_f32(const cvx_t2s_prefill_attention* p, cvx_stream_t s)
{
    CVX_REQUIRE(p != nullptr && p->struct_size == sizeof(cvx_t2s_prefill_attention), "prefill attention: struct_size must be sizeof(cvx_t2s_prefill_attention)");
    CVX_REQUIRE(p->n >= 1 && p->heads >= 1 && p->rows >= 0 && p->max_q >= 0 && p->max_q <= p->rows,
                "prefill attention: bad shape n=%d heads=%d rows=%lld max_q=%d", p->n, p->heads, (long long)p->rows, p->max_q);
    if (p->rows == 0) return CVX_OK;
    CVX_REQUIRE(p->q && p->k && p->v && p->out && p->cu && p->kbase && (p->causal || p->nk), "prefill attention: null pointer");
    CVX_REQUIRE(p->max_q >= 1, "prefill attention: max_q = 0 with %lld rows", (long long)p->rows);
    CVX_REQUIRE(p->ldq >= (int64_t)p->heads * HD && p->ldkv >= (int64_t)p->heads * HD && p->ldq % 4 == 0 && p->ldkv % 4 == 0,
                "prefill attention: row strides must hold heads * 64 floats and be multiples of 4");
    CVX_REQUIRE((((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v | (uintptr_t)p->out) & 15) == 0,
                "prefill attention: pointers must be 16-byte aligned");
    PrefillAttn a;
    a.q = p->q; a.k = p->k; a.v = p->v; a.out = p->out;
    a.cu = p->cu; a.kbase = p->kbase; a.nk = p->nk;
    a.ldq = p->ldq; a.ldkv = p->ldkv;
    a.H = p->heads; a.n_groups = p->n * p->heads; a.n_qt = (p->max_q + QB - 1) / QB; a.causal = p->causal ? 1 : 0;
    a.scale_log2e = p->scale * 1.44269504088896340736f;
    const int64_t blocks = (int64_t)((a.n_groups + 7) / 8) * 8 * a.n_qt;
    CVX_REQUIRE(blocks <= 0x7fffffff, "prefill attention: too many blocks");
    hipLaunchKernelGGL(t2s_prefill_attention_kernel, dim3((unsigned)blocks), dim3(256), 0, cvx_hip_stream(s), a);
    CVX_CHECK_LAUNCH("cvx_t2s_prefill_attention_f32");
    return CVX_OK;
}

extern "C" int cvx_t2s_prefill_guidance_f32(float* logits, const int32_t* null_row, const float* scale, int64_t rows, int32_t width,
                                            cvx_stream_t s)
{
    CVX_REQUIRE(logits && null_row && scale, "prefill guidance: null pointer");
    CVX_REQUIRE(rows >= 0 && rows <= 0x7fffffff && width >= 1, "prefill guidance: bad shape rows=%lld width=%d", (long long)rows, width);
    if (rows == 0) return CVX_OK;
    hipLaunchKernelGGL(t2s_prefill_guidance_kernel, dim3((unsigned)rows), dim3(256), 0, cvx_hip_stream(s), logits, null_row, scale, rows, width);
    CVX_CHECK_LAUNCH("cvx_t2s_prefill_guidance_f32");
    return CVX_OK;
}
