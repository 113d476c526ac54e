// Split-precision flash attention (gfx950): the same algorithm and register choreography as attention_f32.hip
// (reference attend.py:108-126 without the T x T score tensor), but both contractions run on
// v_mfma_f32_32x32x16_f16 with every operand an (fp16 hi, fp16 lo) pair and three products per tile
//     q.k ~= k_hi*q_hi + k_hi*q_lo + k_lo*q_hi        p.v ~= v_hi*p_hi + v_hi*p_lo + v_lo*p_hi     (fp32 accumulate)
// 24 MFMAs of 32 cycles per 32-key tile and wave instead of 64 MFMAs of 64 cycles.
//
// Inputs come pre-split from the to_qkv GEMM epilogue (cvx_gemm_f16x3, QKV mode):
//   qk_hi/qk_lo [Bt*T, 2*H*64]  q | k after RoPE, row-major;
//   vt_hi/vt_lo [Bt*H*64, Tp]   v transposed per (sequence, head): row = head dim, column = frame slot (inside
//                               every 16 frames the four-frame groups are stored in the order 0, 2, 1, 3)
// so that every tile (K: 32 keys x 64 dims, V^T: 64 dims x 32 keys; hi and lo) is a set of contiguous rows that
// go global -> LDS by DMA - no staging registers, no LDS writes by the waves.  LDS tiles are XOR-swizzled on
// the DMA source address (K: chunk ^ ((row >> 1) & 7) over 128-byte rows; V^T: chunk ^ ((row >> 2) & 3) over
// 64-byte rows) so that all fragment reads are conflict-free ds_read_b128.
//
// S^T = K.Q^T keeps a query's scores in one lane pair; P is split in registers and used directly as the B
// operand of O^T += V^T.P^T: the k-slot order of that MFMA is chosen to be exactly the key order the S^T
// accumulator registers already have (registers 8s..8s+7 of lane half g hold keys 16s+4g+{0..3} and
// 16s+8+4g+{0..3}); the producer stores V^T with exactly those eight keys adjacent (frame-slot order above), so a
// V^T fragment is one 16-byte read and P never moves between lanes.
#include "cvx_common.h"
#include <stdlib.h>

namespace {

typedef _Float16 f16;
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int HD = 64, KT = 32;             // queries per block: 32 per wave and query set, NW waves (128; 64 when key-split; 256 with two sets)
constexpr int TILE = KT * HD;                 // halves per operand tile (4 KiB)
constexpr int STAGE = 4 * TILE;               // Khi | Klo | Vthi | Vtlo
constexpr int VALU_PER_MFMA = 6;              // softmax instructions woven into one MFMA gap of the two-set form (24 of its 32 cycles)

__device__ __forceinline__ void glds16(const void* g, void* lds_wave_base)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(uintptr_t)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ f16x8 gload8h(const f16* p)
{
    typedef const f16x8 __attribute__((address_space(1)))* gp;
    return *reinterpret_cast<gp>(reinterpret_cast<uintptr_t>(p));
}

__device__ __forceinline__ void store_split4(f16* hi, f16* lo, int64_t off, const f32x4 o, CvxSat& amax)
{
    cvx_amax4(amax, o);
    // lo == hi + 32: INTERLEAVED pair, [hi 32 | lo 32] per block of 32 values (one 128-byte line per K-step and row for
    // the consumer GEMM's DMA); the mapping is a function of the flat offset because every row is a multiple of 32 wide
    if (lo == hi + 32) off = ((off >> 5) << 6) | (off & 31);
    f16x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x = fminf(fmaxf(o[e], -65504.f), 65504.f);
        h[e] = (f16)x;
        l[e] = (f16)(x - (float)h[e]);
    }
    *reinterpret_cast<f16x4*>(hi + off) = h;
    if (lo) *reinterpret_cast<f16x4*>(lo + off) = l;      // lo == NULL: hi halves only
}

// NT = 3: split operands, three products.  NT = 1: hi halves only (plain fp16 operands, fp32 accumulate and softmax).
constexpr int ATT_WAVES = 2;                       // blocks per CU asked of the compiler (launch bounds) for the one-group form
// NW = waves per block (4, or 2 in the key-split form), 32 queries each.  The K / V^T tiles a block streams through LDS are
// shared by its waves.  Round-3 ablations (tools/archive/attn_ablate.py, Bt = 16,
// T = 1000, H = 16, NW = 4): DMA switched off after the first tile 177 instead of 211 us and 0.233
// instead of 0.286 J (on zero operands, i.e. at full clock, 130 instead of 159 us); no LDS fragment reads -7 %; no
// v_exp_f32 -1 %; no P.V MFMAs 140 us; no K.Q MFMAs 134 us.  Halving the DMA BYTES (NW = 8) does not buy the DMA-off time.
// KS = key-split groups per block (1, 2 or 3; NW = 4): a SHORT launch - one utterance: 2 x 16 (sequence, head) pairs x 4 query
// tiles = 128 blocks of one wave per SIMD, each walking all key tiles in a dependent chain of ~1.45 us per tile (23 us at
// T = 500, while the same wave-tiles take 0.44 us each at three waves per SIMD) - gets KS x 4 waves per block: group s walks
// key tiles s, s + KS, ... through its own two-stage ring with its own running (m, l, O), and group 0 merges the groups' states
// through LDS in the fixed order 0, 1, 2 (the flash-decoding combine: O = sum O_s 2^(m_s - m), l likewise) before it normalises
// and stores.  The chain shortens KS-fold and every SIMD holds KS waves to overlap.
// QS = query sets per wave (1, or 2 in the 256-query form; KS = 1, NW = 4): the wave owns 64 queries as two sets of 32 with their
// own (Q fragments, m, l, O).  Per key tile it reads the K fragments once and runs both sets' S^T chains on them, and reads the
// V^T fragments once for both sets' O^T products: per MFMA half the ds_read_b128, half the L2 -> LDS bytes and half the barriers
// and vmcnt drains of QS = 1.  The straight-line order is S^T(0), S^T(1), softmax(0), P.V(0), softmax(1), P.V(1), so that a set's
// softmax (VALU) has the other set's MFMAs to run under inside the wave.  Every query sees the sums of QS = 1 in the same order, so
// its output bits do not depend on the form.  Code-object metadata (-O3): <3,4,1,2> 244 VGPRs, no scratch (private
// segment 0), 32 KiB of LDS: two blocks per CU (tests/test_attention_form_d.py reads these from the built library).  The three-term
// form is close to the budget of 256: see the notes at zero16, k0 / v0 and te.
template <int NT, int NW, int KS = 1, int QS = 1>
__global__ __launch_bounds__(64 * NW * KS, (KS > 1 ? (NW * KS + 3) / 4 : ATT_WAVES)) void attention_f16x3_kernel(const f16* __restrict__ qk_hi, const f16* __restrict__ qk_lo,
                                                                const f16* __restrict__ vt_hi, const f16* __restrict__ vt_lo,
                                                                float* __restrict__ out, f16* __restrict__ out_hi, f16* __restrict__ out_lo,
                                                                int T, int Tp, int H, int n_groups, int n_qt, float scale_log2e,
                                                                const float* __restrict__ qk_scale, const float* __restrict__ v_scale,
                                                                const float* __restrict__ out_scale, const int* __restrict__ cu_seqlens,
                                                                uint32_t* __restrict__ sat)
{
    // activation pre-scales (device scalars, powers of two): scores carry qk_scale^2, O carries v_scale
    static_assert(QS == 1 || (QS == 2 && KS == 1 && NW == 4), "two query sets per wave: 4 waves, one key group");
    if (qk_scale) { const float q = *qk_scale; scale_log2e /= q * q; }
    __shared__ __attribute__((aligned(16))) f16 smem_all[2 * STAGE * KS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wall = tid >> 6, ks = KS > 1 ? wall / NW : 0, wid = KS > 1 ? wall % NW : wall;     // key group, query wave
    f16* const smem = smem_all + ks * 2 * STAGE;
    const int g = lane >> 5, l31 = lane & 31;
    const int grp = (blockIdx.x / (8 * n_qt)) * 8 + (blockIdx.x & 7);      // same (batch, head) -> same XCD
    if (grp >= n_groups) return;
    const int head = grp % H, b = grp / H;
    constexpr int QB = 32 * NW * QS;
    const int q_blk = ((blockIdx.x >> 3) % n_qt) * QB;
    const int64_t ldqk = (int64_t)2 * H * HD;
    // Key window [kc0, kc1) in V^T COLUMN coordinates; the q|k row of column c is c + roff.
    //   equal-length batch: every (sequence, head) has its own V^T rows, columns 0 .. T-1 (+ zero padding up to Tp);
    //   ragged batch (cu_seqlens): ONE V^T row set per head over all M packed rows (the to_qkv epilogue ran with
    //     rope_T = M), sequence b = columns [cu[b], cu[b+1]).  Key tiles stay aligned to 32 GLOBAL columns (16-byte DMA
    //     pieces, frame-slot groups of 16), so the first and the last tile of a sequence may contain a neighbour's keys:
    //     they are masked like the keys >= T of the last tile (acoustic.py:313: an utterance only ever sees itself).
    int kc0 = 0, kc1 = T, vt_grp = b * H + head;
    int64_t roff = (int64_t)b * T;
    if (cu_seqlens) {
        kc0 = cu_seqlens[b]; kc1 = cu_seqlens[b + 1]; roff = 0; vt_grp = head;
        if (q_blk >= kc1 - kc0) return;            // block-uniform: the grid is sized for the longest sequence
    }
    const int Tb = kc1 - kc0;

    // ---- Q fragments (B operand of S^T): lane (q = l31, g) holds d = 16s + 8g .. +7 for s = 0..3, hi and lo
    // (query set u of wave w: queries q_blk + 32 * (QS * w + u) + l31)
    // query_row: row of the query of set u in the packed tensors, and whether the query exists, for a thread index
    auto query_row = [&](const int t, const int u, bool& valid) __attribute__((always_inline)) {
        int qrow = q_blk + (KS > 1 ? (t >> 6) % NW : t >> 6) * (32 * QS) + (t & 31) + 32 * u;
        valid = qrow < Tb;
        if (!valid) qrow = Tb - 1;
        return roff + kc0 + qrow;
    };
    f16x8 qh[QS][4], ql[QS][4];
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        bool valid;
        const int64_t off = query_row(tid, u, valid) * ldqk + head * HD + 8 * g;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qh[u][s] = gload8h(qk_hi + off + 16 * s);
            if constexpr (NT == 3) ql[u][s] = gload8h(qk_lo + off + 16 * s);
        }
    }

    // ---- DMA sources.  NW = 4: wave w fetches K rows [8w, 8w+8) (hi, lo) and V^T rows [16w, 16w+16) (hi, lo): 4 pieces per
    // tile and wave.  NW = 2 (64-query blocks of the key-split form): every wave fetches two of the four row groups of K and of V^T.
    constexpr int PW = NW == 2 ? 2 : 1;                                     // row groups per wave
    const int wq = NW == 2 ? 2 * wid : (wid & 3);
    int k_r[PW], k_c[PW], v_r[PW], v_c[PW];
    int64_t k_col[PW], v_row[PW];
#pragma unroll
    for (int pp = 0; pp < PW; ++pp) {
        k_r[pp] = 8 * (wq + pp) + (lane >> 3);                              // key row inside the tile
        k_c[pp] = (lane & 7) ^ ((k_r[pp] >> 1) & 7);                        // source chunk for LDS chunk (lane & 7)
        k_col[pp] = (int64_t)H * HD + head * HD + 8 * k_c[pp];
        v_r[pp] = 16 * (wq + pp) + (lane >> 2);                             // head-dim row inside the tile
        v_c[pp] = (lane & 3) ^ ((v_r[pp] >> 2) & 3);
        v_row[pp] = ((int64_t)vt_grp * HD + v_r[pp]) * Tp + 8 * v_c[pp];
    }
    auto issue = [&](int key0, int stage) {
        f16* S = smem + stage * STAGE;
#pragma unroll
        for (int pp = 0; pp < PW; ++pp) {
            const int key = min(max(key0 + k_r[pp], kc0), kc1 - 1);
            const int64_t ko = (roff + key) * ldqk + k_col[pp];
            glds16(qk_hi + ko, S + 8 * (wq + pp) * HD);
            if constexpr (NT == 3) glds16(qk_lo + ko, S + TILE + 8 * (wq + pp) * HD);
            const int64_t vo = v_row[pp] + key0;
            glds16(vt_hi + vo, S + 2 * TILE + 16 * (wq + pp) * KT);
            if constexpr (NT == 3) glds16(vt_lo + vo, S + 3 * TILE + 16 * (wq + pp) * KT);
        }
    };

    // ---- fragment offsets (halves)
    int koff[4];                                   // K rows are 64 halves; chunk (2s+g) ^ ((row>>1)&7)
#pragma unroll
    for (int s = 0; s < 4; ++s) koff[s] = l31 * HD + 8 * ((2 * s + g) ^ ((l31 >> 1) & 7));
    int voff[2];                                   // V^T rows are 32 halves; chunk (2s + g) ^ ((row>>2)&3)
#pragma unroll
    for (int s = 0; s < 2; ++s) voff[s] = l31 * KT + 8 * ((2 * s + g) ^ ((l31 >> 2) & 3));

    // QS = 2: a wave whose 64 queries all lie past the sequence's end (up to three of the last block's four) only streams its share
    // of the tiles: form D then never runs more query sets through the matrix pipe than the 128-query forms do
    const bool idle = QS > 1 && __builtin_amdgcn_readfirstlane(q_blk + (tid >> 6) * (32 * QS)) >= Tb;
    f32x16 o0[QS], o1[QS];
    float m_run[QS], l_run[QS];
#pragma unroll
    for (int u = 0; u < QS; ++u) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[u][r] = 0.f; o1[u][r] = 0.f; }
        m_run[u] = -1e30f; l_run[u] = 0.f;
    }
    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
    asm volatile("" : "+v"(zero16));          // opaque to the optimiser: stays one register block instead of 16 movs per tile

    // (a stage of two key tiles - one barrier per 64 keys - was measured slower: 64 KiB of LDS drops the kernel
    //  from 3 to 2 blocks per CU)
    // (a 3-stage ring - tiles requested two ahead - measured the same: the loop is not DMA-latency bound)
    const int tile0 = kc0 / KT, ntiles = (kc1 + KT - 1) / KT - tile0;
    if (KS == 1 || ks == 0) issue(tile0 * KT, 0);
    f16x8 kfh[4], kfl[4];                         // K fragments of the running tile
    f16x8 vfh[2][2], vfl[2][2];                   // V^T fragments [s][dt]
    if (KS > 1 && ks > 0 && ks < ntiles) issue((tile0 + ks) * KT, 0);      // (group 0's first tile was requested above)
    const int n_it = KS > 1 ? (ntiles + KS - 1) / KS : ntiles;
    for (int jt = 0; jt < n_it; ++jt) {
        const int it = KS > 1 ? jt * KS + ks : jt;
        const int cur = jt & 1, key0 = (tile0 + it) * KT;
        if (KS > 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                   // this group's tile landed (all four waves); its other stage is free
            if (it + KS < ntiles) issue(key0 + KS * KT, cur ^ 1);
            if (it >= ntiles) continue;                     // (group-uniform: a group past its last tile only keeps the barriers company)
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                   // tile `it` landed everywhere; stage cur^1 is free
            if (it + 1 < ntiles) issue(key0 + KT, cur ^ 1);
            if constexpr (QS > 1) if (idle) continue;       // (the wave still fetched its pieces of the tile and met the barrier)
        }
        const f16* S = smem + cur * STAGE;

        // ---- S^T = K . Q^T  (3 products per 16-wide d slice), ONE accumulator: the matrix pipe forwards the result of an
        // MFMA to a dependent MFMA on the same accumulator, so the chain costs nothing and the adds that would merge
        // per-term accumulators disappear (measured: 1 accumulator 260 us, 3 accumulators 272 us, 2: 285 us).
        // The first MFMA of the chain takes its C operand from a zero register block kept live over the loop.
        f32x16 sacc[QS];
        // QS = 2 carries only slice 0's fragment offsets over the loop and derives the others here (the slice index only flips bits
        // of the swizzled chunk: koff[s] == koff[0] ^ 16 s, voff[1] == voff[0] ^ 16): four registers the two query sets need
        int k0 = koff[0], v0 = voff[0];
        if constexpr (QS > 1) asm volatile("" : "+v"(k0), "+v"(v0));
#pragma unroll                                     // all K fragments first (8 reads in flight), then the MFMA chain
        for (int s = 0; s < 4; ++s) {
            const int ko = QS == 1 ? koff[s] : k0 ^ (16 * s);
            kfh[s] = *reinterpret_cast<const f16x8*>(S + ko);
            if constexpr (NT == 3) kfl[s] = *reinterpret_cast<const f16x8*>(S + TILE + ko);
        }
        // (QS = 2: the chain starts from the inline constant 0 instead - 16 registers the two sets need elsewhere)
        auto chain = [&](const int u) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if constexpr (NT == 3) {
                    sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfl[s], qh[u][s], s == 0 ? (QS == 1 ? zero16 : f32x16{}) : sacc[u], 0, 0, 0);
                    sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfh[s], ql[u][s], sacc[u], 0, 0, 0);
                    sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfh[s], qh[u][s], sacc[u], 0, 0, 0);
                } else {
                    sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfh[s], qh[u][s], s == 0 ? (QS == 1 ? zero16 : f32x16{}) : sacc[u], 0, 0, 0);
                }
            }
        };
        chain(0);

        // ---- online softmax (this lane: 16 keys of query l31; partner lane^32 holds the other 16).
        // The running max m_run is kept in the scaled log2 domain; scores stay raw and the scale is folded into one
        // fma per element: p = exp2(s*c - m).  Only the last tile (ragged batches: and the first) can contain keys outside the sequence (wave-uniform branch), and
        // the 32 accumulator rescales are skipped when no lane's max moved (alpha == 1 exactly - also wave-uniform).
        f16x8 ph[QS][2], pl[QS][2];
        float alpha[QS];
        bool moved[QS];
        auto mask = [&](const int u) __attribute__((always_inline)) {
            f32x16& sc = sacc[u];
            if (key0 + KT > kc1 || key0 < kc0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kk = key0 + mfma32_row(r, lane);
                    if (kk >= kc1 || kk < kc0) sc[r] = -1e30f;
                }
            }
        };
        auto probs = [&](const int u) __attribute__((always_inline)) {
            f32x16& sc = sacc[u];
            float mx = sc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sc[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * scale_log2e;          // scale > 0: max commutes with it
            const float m_new = fmaxf(m_run[u], mx);
            moved[u] = m_new != m_run[u];
            alpha[u] = __builtin_amdgcn_exp2f(m_run[u] - m_new);
            m_run[u] = m_new;
            float psum = 0.f;
            {
                // two probabilities at a time: one packed RNE conversion for the hi halves, the residuals straight from the
                // packed register with v_fma_mix_f32 (fp16 source, fp32 result: pv - hi, exact), one packed conversion for lo
                typedef float f32x2 __attribute__((ext_vector_type(2)));
                typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                u32x4 hw[2], lw[2];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float a0 = fmaf(sc[2 * j], scale_log2e, -m_new), a1 = fmaf(sc[2 * j + 1], scale_log2e, -m_new);
                    const float p0 = __builtin_amdgcn_exp2f(a0), p1 = __builtin_amdgcn_exp2f(a1);
                    psum += p0 + p1;                 // (pairs first: 8 dependent adds instead of 16)
                    const f16x2 h2 = __builtin_convertvector(f32x2{p0, p1}, f16x2);
                    const unsigned int hb = __builtin_bit_cast(unsigned int, h2);
                    hw[j >> 2][j & 3] = hb;
                    if constexpr (NT == 3) {
                        float r0, r1;
                        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hb), "v"(p0));
                        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hb), "v"(p1));
                        const f16x2 l2 = __builtin_convertvector(f32x2{r0, r1}, f16x2);
                        lw[j >> 2][j & 3] = __builtin_bit_cast(unsigned int, l2);
                    }
                }
                ph[u][0] = __builtin_bit_cast(f16x8, hw[0]); ph[u][1] = __builtin_bit_cast(f16x8, hw[1]);
                if constexpr (NT == 3) { pl[u][0] = __builtin_bit_cast(f16x8, lw[0]); pl[u][1] = __builtin_bit_cast(f16x8, lw[1]); }
            }
            l_run[u] = l_run[u] * alpha[u] + psum;
        };
        auto rescale = [&](const int u) __attribute__((always_inline)) {
            if (__any(moved[u])) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { o0[u][r] *= alpha[u]; o1[u][r] *= alpha[u]; }
            }
        };
        // one MFMA, then VALU_PER_MFMA vector instructions of the other set's softmax, N times: the softmax of one set is issued in
        // the gaps of the other set's products instead of after them
        auto weave = [&](const int n) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < n; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                  // MFMA
                __builtin_amdgcn_sched_group_barrier(0x402, VALU_PER_MFMA, 0);      // VALU and transcendentals
            }
        };

        // ---- O^T += V^T . P^T
        const f16* Vh = S + 2 * TILE;
        const f16* Vl = S + 3 * TILE;
        auto load_v = [&](const int s) __attribute__((always_inline)) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const int vo = QS == 1 ? voff[s] : v0 ^ (16 * s);
                vfh[s][dt] = *reinterpret_cast<const f16x8*>(Vh + dt * 32 * KT + vo);
                if constexpr (NT == 3) vfl[s][dt] = *reinterpret_cast<const f16x8*>(Vl + dt * 32 * KT + vo);
            }
        };
        auto pv = [&](const int u, const int s) __attribute__((always_inline)) {
            f16x8 (&vhh)[2] = vfh[s];
            f16x8 (&vll)[2] = vfl[s];
            // interleave the two O^T tiles: consecutive MFMAs alternate accumulators
            if constexpr (NT == 3) {
                o0[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vll[0], ph[u][s], o0[u], 0, 0, 0);
                o1[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vll[1], ph[u][s], o1[u], 0, 0, 0);
                o0[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vhh[0], pl[u][s], o0[u], 0, 0, 0);
                o1[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vhh[1], pl[u][s], o1[u], 0, 0, 0);
            }
            o0[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vhh[0], ph[u][s], o0[u], 0, 0, 0);
            o1[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vhh[1], ph[u][s], o1[u], 0, 0, 0);
        };
        mask(0);
        if constexpr (QS == 1) {
            probs(0); rescale(0);
#pragma unroll
            for (int s = 0; s < 2; ++s) { load_v(s); pv(0, s); }
        } else {
            // set 1's S^T chain under set 0's softmax, set 0's products under set 1's softmax (the wave-uniform branches of the
            // masking and of the rescale bound the straight-line pieces).  The V^T fragments are read once, when the K fragments
            // are dead, and serve both sets.
            chain(1); probs(0); weave(NT == 3 ? 12 : 4);
            rescale(0);
            load_v(0); load_v(1);
            mask(1);
            pv(0, 0); pv(0, 1); probs(1); weave(NT == 3 ? 12 : 4);
            rescale(1);
            pv(1, 0); pv(1, 1);
        }
    }

    if constexpr (KS > 1) {
        // merge the key groups' states: groups 1 .. KS-1 park (m, l, O) in LDS (the rings are dead), group 0 folds them in order
        __syncthreads();
        f32x4* const X = reinterpret_cast<f32x4*>(smem_all);
        if (ks > 0) {
            f32x4* const dst = X + ((size_t)((ks - 1) * NW + wid) * 9) * 64 + lane;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                dst[q4 * 64] = f32x4{o0[0][4 * q4], o0[0][4 * q4 + 1], o0[0][4 * q4 + 2], o0[0][4 * q4 + 3]};
                dst[(4 + q4) * 64] = f32x4{o1[0][4 * q4], o1[0][4 * q4 + 1], o1[0][4 * q4 + 2], o1[0][4 * q4 + 3]};
            }
            dst[8 * 64] = f32x4{m_run[0], l_run[0], 0.f, 0.f};
        }
        __syncthreads();
        if (ks > 0) return;
#pragma unroll
        for (int s2 = 1; s2 < KS; ++s2) {
            const f32x4* const src = X + ((size_t)((s2 - 1) * NW + wid) * 9) * 64 + lane;
            const f32x4 ml = src[8 * 64];
            const float m_new = fmaxf(m_run[0], ml[0]);
            const float fa = __builtin_amdgcn_exp2f(m_run[0] - m_new), fb = __builtin_amdgcn_exp2f(ml[0] - m_new);
            m_run[0] = m_new;
            l_run[0] = l_run[0] * fa + ml[1] * fb;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const f32x4 a = src[q4 * 64], c = src[(4 + q4) * 64];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o0[0][4 * q4 + e] = o0[0][4 * q4 + e] * fa + a[e] * fb;
                    o1[0][4 * q4 + e] = o1[0][4 * q4 + e] * fa + c[e] * fb;
                }
            }
        }
    }
    if constexpr (QS > 1) if (idle) return;            // nothing to store, and no normaliser to judge
    float l_tot[QS], inv[QS];
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        l_tot[u] = l_run[u] + __shfl_xor(l_run[u], 32, 64);
        inv[u] = 1.0f / l_tot[u] / (v_scale ? *v_scale : 1.f);             // fp32 output: the true value
    }
    const float osc = out_scale ? *out_scale : 1.f;                        // split output: times the consumer's pre-scale
    CvxSat amax;
    // QS = 2: the output rows are derived again from a thread index the optimiser cannot connect with the first one, instead of six
    // registers carried over the loop (which needs every one of its 256)
    int te = tid;
    if constexpr (QS > 1) asm volatile("" : "+v"(te));
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        bool valid;
        const int64_t q_grow = query_row(te, u, valid);
        if (valid) {
            const int64_t o_off = q_grow * (H * HD) + head * HD + 4 * ((te & 63) >> 5);
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                f32x4 a, c;
#pragma unroll
                for (int e = 0; e < 4; ++e) { a[e] = o0[u][4 * gq + e] * inv[u]; c[e] = o1[u][4 * gq + e] * inv[u]; }
                if (out) {
                    *reinterpret_cast<f32x4*>(out + o_off + 8 * gq) = a;
                    *reinterpret_cast<f32x4*>(out + o_off + 32 + 8 * gq) = c;
                }
                if (out_hi) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] *= osc; c[e] *= osc; }
                    store_split4(out_hi, out_lo, o_off + 8 * gq, a, amax);
                    store_split4(out_hi, out_lo, o_off + 32 + 8 * gq, c, amax);
                }
            }
        }
        // a non-finite normaliser (overflowed scores, all-masked row) also means the result cannot be trusted: flag it
        if (!(l_tot[u] > 0.f && l_tot[u] < __builtin_inff())) amax.bad = true;
    }
    cvx_sat_commit(sat, amax);
}

}  // namespace

// Which attention_f16x3_kernel<NT, NW, KS> a launch takes (pure host arithmetic; launch_attention_f16x3 and the exported
// cvx_attention_f16x3_form both call it).  T: frames per sequence, or the LONGEST sequence of a ragged batch; q_rows: query rows of
// the launch.  Returns the form and writes queries per block, key groups and query waves per block (form D: 256, 1, 4 - its waves own
// two query sets each).
static int attention_f16x3_form(int32_t n_seq, int32_t T, int64_t q_rows, int32_t H, bool single, int* query_block, int* key_groups, int* query_waves)
{
    // Forms A, B: 128-query blocks (4 waves, three blocks per CU).  (A removed geometry of 256-query blocks as EIGHT waves of 32 queries -
    // half the L2 -> LDS tile traffic per score, one block per CU - measured 3 % slower than that: 218.6 vs 212.5 us, same joules; on
    // zero operands 182 vs 159 us.  Form D below is 256 queries on FOUR waves, two blocks per CU.)
    int qb = 128;
    const int64_t n_groups = (int64_t)n_seq * H;
    const int64_t blocks128 = ((n_groups + 7) / 8) * 8 * ((T + 127) / 128);       // grid of the 128-query forms: decides between B and C
    // key-split groups for short launches (see the kernel): fewer than 2048 query rows = at most one 128-query block per CU (96 KiB of
    // LDS with three groups).
    int ksplit = 1, nwk = 4, form = CVX_ATT_FORM_A;
    // 256-query blocks of 4 waves x two query sets (QS = 2, two blocks per CU) once they fill the chip's 2 x 256 slots at least once:
    // half the fragment reads, tile traffic and barriers per MFMA (see the kernel; measurements in DESIGN.md section 4.4).  Equal-length
    // and ragged launches alike; below that, the rule is what it was.
    // Three-term launches only: the single-term twin of this geometry measured SLOWER than form A1 (16 x 1000 x 16: 118.2 - 118.9 against
    // 113.8 - 116.3 us; T = 777: 92 against 86 us - its loop is short of registers' worth of work to share), so A1 keeps those.
    if (!single && n_groups * ((T + 255) / 256) >= 512) { qb = 256; form = CVX_ATT_FORM_D; }
    else if (T >= 4 * KT && q_rows < 2048) {
        ksplit = 3; form = CVX_ATT_FORM_B;
        // half of the chip's SIMDs hold no wave at all when the 128-query blocks number fewer than 128: 64-query blocks (two query waves,
        // four key groups: 8 waves per block) put a wave on every SIMD
        if (blocks128 <= 128) { nwk = 2; ksplit = 4; qb = 64; form = CVX_ATT_FORM_C; }
    }
    *query_block = qb; *key_groups = ksplit; *query_waves = nwk;
    return form + (single ? CVX_ATT_FORM_SINGLE_TERM : 0);
}

static int launch_attention_f16x3(const uint16_t* qk_hi, const uint16_t* qk_lo, const uint16_t* vt_hi, const uint16_t* vt_lo,
                                  float* out, uint16_t* out_hi, uint16_t* out_lo, const int32_t* cu_seqlens_dev,
                                  int32_t Bt, int32_t T, int64_t cols, int32_t Tp, int32_t H, float scale,
                                  const float* qk_scale_dev, const float* v_scale_dev, const float* out_scale_dev, cvx_stream_t s)
{
    // T: frames per sequence (equal-length batch) or the LONGEST sequence (ragged batch); cols: V^T columns in use
    const bool single = (qk_lo == nullptr);        // hi halves only: plain fp16 operands, one product
    CVX_REQUIRE(qk_hi && vt_hi && ((qk_lo == nullptr) == (vt_lo == nullptr)) && (out || out_hi) &&
                (out_hi || !out_lo) && (single || (out_hi == nullptr) == (out_lo == nullptr)),
                "attention_f16x3: null pointer");
    CVX_REQUIRE(Bt >= 0 && T > 0 && H > 0 && Tp % 8 == 0 && Tp >= ((cols + KT - 1) / KT) * KT,
                "attention_f16x3: bad shape Bt=%d T=%d Tp=%d H=%d (Tp must be a multiple of 8 and >= the V^T columns in use rounded up to 32)", Bt, T, Tp, H);
    CVX_REQUIRE((((uintptr_t)qk_hi | (uintptr_t)qk_lo | (uintptr_t)vt_hi | (uintptr_t)vt_lo) & 15) == 0,
                "attention_f16x3: inputs must be 16-byte aligned");
    if (Bt == 0) return CVX_OK;
    int qb, ksplit, nwk;
    const int64_t q_rows = cu_seqlens_dev ? cols : (int64_t)Bt * T;             // query rows of the launch
    attention_f16x3_form(Bt, T, q_rows, H, single, &qb, &ksplit, &nwk);
    const int n_qt = (T + qb - 1) / qb;
    const int n_groups = Bt * H;
    const dim3 grid((unsigned)(((n_groups + 7) / 8) * 8 * n_qt));
    if (out_hi) CVX_REQUIRE_SAT(s);
    uint32_t* sat = cvx_sat_flag_for(s);
#define CVX_ATT_LAUNCH_KS(NT_, KS_) CVX_ATT_LAUNCH_KW(NT_, 4, KS_)
#define CVX_ATT_LAUNCH_KW(NT_, NW_, KS_)                                                                                                  \
    hipLaunchKernelGGL((attention_f16x3_kernel<NT_, NW_, KS_>), CVX_ATT_ARGS(NW_, KS_))
#define CVX_ATT_ARGS(NW_, KS_)                                                                                                            \
    grid, dim3(64 * NW_ * KS_), 0, cvx_hip_stream(s),                                                                                     \
        reinterpret_cast<const f16*>(qk_hi), reinterpret_cast<const f16*>(qk_lo),                                                         \
        reinterpret_cast<const f16*>(vt_hi), reinterpret_cast<const f16*>(vt_lo),                                                         \
        out, reinterpret_cast<f16*>(out_hi), reinterpret_cast<f16*>(out_lo),                                                              \
        T, Tp, H, n_groups, n_qt, scale * 1.44269504088896340736f, qk_scale_dev, v_scale_dev, out_scale_dev, cu_seqlens_dev, sat
    if (qb == 256) hipLaunchKernelGGL((attention_f16x3_kernel<3, 4, 1, 2>), CVX_ATT_ARGS(4, 1));
    else if (nwk == 2) { if (single) CVX_ATT_LAUNCH_KW(1, 2, 4); else CVX_ATT_LAUNCH_KW(3, 2, 4); }
    else if (ksplit == 3) { if (single) CVX_ATT_LAUNCH_KS(1, 3); else CVX_ATT_LAUNCH_KS(3, 3); }
    else if (single) CVX_ATT_LAUNCH_KS(1, 1);
    else CVX_ATT_LAUNCH_KS(3, 1);
#undef CVX_ATT_LAUNCH_KS
#undef CVX_ATT_LAUNCH_KW
#undef CVX_ATT_ARGS
    CVX_CHECK_LAUNCH("cvx_attention_f16x3");
    return CVX_OK;
}

extern "C" int cvx_attention_f16x3_scaled(const uint16_t* qk_hi, const uint16_t* qk_lo, const uint16_t* vt_hi, const uint16_t* vt_lo,
                                          float* out, uint16_t* out_hi, uint16_t* out_lo,
                                          int32_t Bt, int32_t T, int32_t Tp, int32_t H, float scale,
                                          const float* qk_scale_dev, const float* v_scale_dev, const float* out_scale_dev, cvx_stream_t s)
{
    return launch_attention_f16x3(qk_hi, qk_lo, vt_hi, vt_lo, out, out_hi, out_lo, nullptr, Bt, T, T, Tp, H, scale,
                                  qk_scale_dev, v_scale_dev, out_scale_dev, s);
}

extern "C" int cvx_attention_f16x3_varlen(const uint16_t* qk_hi, const uint16_t* qk_lo, const uint16_t* vt_hi, const uint16_t* vt_lo,
                                          float* out, uint16_t* out_hi, uint16_t* out_lo, const int32_t* cu_seqlens_dev,
                                          int32_t n_seq, int32_t max_T, int64_t M, int32_t vt_ld, int32_t H, float scale,
                                          const float* qk_scale_dev, const float* v_scale_dev, const float* out_scale_dev, cvx_stream_t s)
{
    CVX_REQUIRE(cu_seqlens_dev && M >= 0 && max_T <= M, "attention_f16x3_varlen: needs cu_seqlens and max_T <= M");
    return launch_attention_f16x3(qk_hi, qk_lo, vt_hi, vt_lo, out, out_hi, out_lo, cu_seqlens_dev, n_seq, max_T, M, vt_ld, H, scale,
                                  qk_scale_dev, v_scale_dev, out_scale_dev, s);
}

extern "C" int cvx_attention_f16x3(const uint16_t* qk_hi, const uint16_t* qk_lo, const uint16_t* vt_hi, const uint16_t* vt_lo,
                                   float* out, uint16_t* out_hi, uint16_t* out_lo,
                                   int32_t Bt, int32_t T, int32_t Tp, int32_t H, float scale, cvx_stream_t s)
{
    return cvx_attention_f16x3_scaled(qk_hi, qk_lo, vt_hi, vt_lo, out, out_hi, out_lo, Bt, T, Tp, H, scale, nullptr, nullptr, nullptr, s);
}

extern "C" int cvx_attention_f16x3_form(int32_t n_seq, int32_t max_T, int64_t q_rows, int32_t H, int32_t single_term,
                                        int32_t* query_block, int32_t* key_groups, int32_t* query_waves)
{
    if (n_seq <= 0 || max_T <= 0 || H <= 0 || q_rows < max_T) return -1;
    int qb, ks, nw;
    const int form = attention_f16x3_form(n_seq, max_T, q_rows, H, single_term != 0, &qb, &ks, &nw);
    if (query_block) *query_block = qb;
    if (key_groups) *key_groups = ks;
    if (query_waves) *query_waves = nw;
    return form;
}
