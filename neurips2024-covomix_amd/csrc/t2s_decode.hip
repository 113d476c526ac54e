// text2semantic autoregressive decode: one token step of the reference's
// TextToSemantic.generate sampling loop (covomix/covomix_model/text2semantic.py:748-820) with a KV cache.
//
// One new position per step: every projection is a matrix-VECTOR product, so the step is bound by streaming the
// decoder weights (CoSingle 60 MB, CoMix 186 MB of fp32 per token step) - an HBM/MALL-bound path, not an MFMA one.
// BATCH: up to 64 decode SLOTS advance together (each at its OWN position, with its own context / cache / eos): a weight row
// is read once per group of 8 slots and multiplied with every slot's vector.  The chain of 34 dependent launches is latency-bound,
// so a step at batch 32 costs little more than at batch 8.  The arithmetic per utterance (summation order included) does not
// depend on the batch size, the slot or the position of the other slots: results are bit-identical to batch 1.
// CONTINUOUS BATCHING (round 6): with a dialogue queue (cvx_t2s_decoder.queue) a slot whose dialogue has sampled its eos (or
// reached its step limit) takes the next pending dialogue INSIDE sample_kernel - no host round trip, no idle slot-steps; the
// per-dialogue buffers (context k/v, uniforms, tokens) are indexed by the dialogue number the slot record carries.  Under guidance a
// slot PAIR decodes a pair of dialogue records (text context, null context) and the even slot refills both.
// Kernels (all fp32, fp32 accumulate):
//   gemv_kernel<MODE>   block = 4 waves, every wave owns TWO output rows (the pairs are chosen so that the epilogue
//                       has both members of a RoPE pair / a GEGLU (value, gate) pair in one wave); the input vector is
//                       staged in LDS once per block, optionally RMS-normalised (F.normalize * sqrt(D) * gamma,
//                       text2semantic.py:143-151) on the way; rows stream with 16-byte loads + a wave reduction.
//   attn_kernel         one block per head over the cached keys (self: roped keys [0, pos]; cross: learned null k/v +
//                       the encoder context, text2semantic.py:253-262); 16 lanes per key for coalesced 256-byte rows.
//   sample_kernel       the logit filter - top-k (:126-132; k from the descriptor) or top-p (:118-124) - + Gumbel argmax (:105-113) from
//                       caller-supplied U(0,1) draws, eos bookkeeping (:803-818), and the embedding of the sampled ids = next step's input.
//                       Its LOGP instantiations (cvx_t2s_decode_steps_scored) also store the log-probability of the step's token and honour
//                       FORCED dialogues, which read given tokens instead of sampling (teacher-forced scoring).
//   sample_per_kernel   sample_kernel with temperature, filter, guidance scale and a forced prefix length read per step from a table row of
//                       the DIALOGUE the slot decodes (cvx_t2s_decode_steps_per_dialogue): utterances with different settings share the slots.
//   sample_mixed_kernel, mixed_schedule_kernel   guided and unguided dialogues in one slot pool (cvx_t2s_decode_steps_mixed): a slot's
//                       role (single / text half / null half) comes from its record, and a one-block launch after the sampling
//                       kernel hands the idle slots the next records - a guided record takes two slots, wherever they are.
//   sample_rules_kernel, sample_mixed_rules_kernel   those two under the HISTORY RULES of the dialogue (cvx_t2s_decode_steps_rules): repetition
//                       penalty, no-repeat n-gram and minimum length from the stream's own token row - per-id marks in LDS (rules_marks), the
//                       ruled row staged in place of the plain one (rules_stage), then the same filter and argmax; rules_rows_kernel: the
//                       rules alone (cvx_t2s_rules_f32).
// BEAM SEARCH (cvx_t2s_beam_steps; the algorithm: include/covomix_hip.h): the B hypotheses of an utterance sit in B neighbouring slots and
// continue from each other's KV caches through an ancestry table - no cache row is ever copied:
//   attn_owner_kernel      attn_kernel's body with key / value j read from the cache of slot owner[j] (the row staged in LDS);
//   beam_shortlist_kernel  per live row the min(B, V) largest log-softmax entries (row_logprob's maximum and sum), in place of sample_kernel;
//   beam_merge_kernel      per utterance the B best of the <= B^3 candidates; writes back-pointers, scores, slot records, the next inputs and
//                          the next ancestry rows;  beam_backtrack_kernel: the back-pointers into token / log-prob rows, once at the end.
// cvx_t2s_beam_queue_steps runs a LIST of utterances through the groups: beam_merge_queue_kernel ends an utterance, takes the next pending
// one from a device-side queue and re-arms the whole group inside the same launch; the history is then kept per utterance
// (beam_backtrack_queue_kernel).
// BEAM SEARCH UNDER GUIDANCE (cvx_t2s_beam_guided_steps, cvx_t2s_beam_guided_queue_steps): a hypothesis is a slot PAIR - slot 2h with the text
// context, slot 2h + 1 with the null context - with one score, one history and one ancestry; the chain and attn_owner_kernel (one block row
// per slot) are those of the beam search:
//   beam_shortlist_guided_kernel   one block per live hypothesis: stage_row's null + (cond - null) * scale over the logits rows of both halves -
//                          the row the guided scoring path takes its log-probs from - then the shortlist;
//   beam_merge_guided_kernel, beam_merge_guided_queue_kernel   beam_merge_step<QUEUE, GUIDED = true>: the selection over hypotheses; slot
//                          records, the next input (one embedding row into both x rows) and the ancestry rows (text row from the parent's text
//                          row, null row from its null row) for both halves; the queue form re-arms both halves of a refilled group.
//                          The back-track kernels are shared: their rows are hypotheses either way.
// BEAM SEARCH UNDER THE HISTORY RULES (cvx_t2s_beam_rules_steps: the four beam chains with no-repeat n-gram and minimum length):
//   beam_shortlist_rules_kernel<QUEUE>, beam_shortlist_guided_rules_kernel<QUEUE>   the shortlists with the hypothesis' own history gathered
//                          along the ancestry table into LDS (beam_history), rules_marks' ban marks over it, and the bans applied to the
//                          log-softmax between the lp pass and the ranking (beam_shortlist<NT, RULES>);
//   beam_merge_*_rules_kernel   beam_merge_step<QUEUE, GUIDED, RULES = true>: a banned shortlist entry (-inf) gives no candidate.
// The same two launches per step; the kernels of the plain chains keep their instruction text.
// ONE BODY PER STEP: the five sampling kernels instantiate sample_step, the four merge kernels beam_merge_step, the two back-track kernels
// beam_backtrack_step.  What such sharing does to a kernel is read from the compiler (tools/kernel_text_diff.py against the parent's
// assembly), not assumed: the default chain's kernels keep their instruction text (tests/test_t2s_code_objects.py holds their resources).
// The reference rotates ALL cached keys again every step with rotary_embedding_torch's interleaved pairs
// (rotary_embedding_torch.py:146-157); rotating a key once at its own position when it enters the cache is the same
// arithmetic.  Interleaved pairs (2i, 2i+1) become half-split pairs (i, i+32) by permuting the rows of to_q / to_k
// inside every head at load time (q.k is invariant under a common permutation) - done by the host packer.
// Positions: the device-side slot records (state[slot][0]); every kernel reads them, so a captured HIP graph of N steps replays as is.
#include "cvx_common.h"

// No implicit a * b + c -> fma contraction in this file: the batch-1 / 2 / 4 / 8 instances of a kernel are REQUIRED to agree
// bitwise per utterance (tests/test_t2s_gpu.py: batched == one-by-one tokens); every fused multiply-add below is an explicit fmaf.
#pragma clang fp contract(off)

namespace {

constexpr int T2S_MAX_KEYS = 4096;
constexpr int T2S_MAX_DIM = 4096;     // floats of the staged input vector (16 KiB of LDS)
constexpr int SR = 8;                 // int32 per slot record / dialogue record (cvx_t2s_decoder.state / .dialogues)
constexpr int T2S_MAX_BATCH = 64;

enum { MODE_QKV = 0, MODE_PLAIN = 1, MODE_RES = 2, MODE_GEGLU = 3, MODE_LOGITS = 4 };

struct GemvArgs {
    const float* W;          // [N, ldw]
    int64_t ldw;
    const float* x;          // input vectors [batch][x_stride], K used
    const float* gamma;      // RMSNorm weight over x (NULL: x is used as is)
    const float* bias;       // [N] or NULL
    float* y;                // output [batch][y_stride]
    int N, K;
    int x_stride, y_stride;
    int64_t cache_stride;    // floats between the k/v caches of two utterances
    // MODE_QKV: rows [0, inner) q, [inner, 2 inner) k, [2 inner, 3 inner) v; RoPE on q/k at position *pos
    int inner;
    const float* rope_cos;   // [max_len, 32]
    const float* rope_sin;
    float* k_cache;          // [max_len, inner]
    float* v_cache;
    const int* state;        // slot records: state[SR * slot + 0] = pos
    int max_len;             // positions >= max_len are clamped (the host never asks for them; keeps a stray call in bounds)
    // slot groups (batch > 8): the batch is ceil(batch / 8) groups of BQ = 8 slots; `gy` blocks share a row block (dispatched back
    // to back on one XCD: L2 hits) and block i of them starts at group i * gl (gl = 1: one group per block)
    int gy, gl, n_blocks;
    // MODE_GEGLU: rows j (value) and j + F (gate), F = N / 2; y[j] for j < F, zero fill up to y_pad
    int y_pad;
    // MODE_LOGITS: `streams` independent slices of the normalised vector: y[s*N + n] = W[n,:] . xn[s*K .. (s+1)*K)
    int streams;
};

// x[l] + x[l ^ o] for o = 8 / 4 / 2 / 1 without an LDS permute: DPP row rotation (xor 8 inside a 16-lane row), the LDS crossbar's swizzle
// (xor 4) and DPP quad permutes fused into the add - the pairings of the xor butterfly exactly, so the same bits as __shfl_xor
__device__ __forceinline__ float xor_add8(float v) { return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, false)); }   // row_ror:8
__device__ __forceinline__ float xor_add4(float v) { return v + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x101F)); }
__device__ __forceinline__ float xor_add2(float v) { return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)); }
__device__ __forceinline__ float xor_add1(float v) { return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)); }

__device__ __forceinline__ float wave_sum(float v)
{
    v += __shfl_xor(v, 32, 64);
    v += __shfl_xor(v, 16, 64);
    return xor_add1(xor_add2(xor_add4(xor_add8(v))));
}

constexpr int PF = 4;                                      // 4 x 256 floats per row in flight (K <= 1024 entirely)
// weight rows: streamed once per token step by one wave each -> non-temporal loads
__device__ __forceinline__ f32x4 wload4(const float* p) { return gload4_nt(p); }
// ACTIVATION reads (x, q, att, h, logits, the state record, cache rows) are plain loads (round 4 measured L1-bypassing loads at
// -36 % on this per-launch path: 147.8 -> 201.2 us per CoSingle step)
__device__ __forceinline__ float aload(const float* p) { return *p; }
__device__ __forceinline__ int aloadi(const int* p) { return *p; }
__device__ __forceinline__ f32x4 aload4(const float* p) { return gload4(p); }

// the two rows of row-pair `pair` (the pairs are chosen so that the epilogue has both members of a RoPE pair / a GEGLU
// (value, gate) pair in one wave)
template <int MODE>
__device__ __forceinline__ bool pair_rows(const GemvArgs& a, int pair, int& r0, int& r1, int& sidx)
{
    sidx = 0;
    if (MODE == MODE_QKV) {
        // pair p -> head-local (h, i): rows base + h*64 + i and + 32 for i in [0, 32); 3*inner/2 pairs in total
        const int per = a.inner / 2;
        const int sec = pair / per, q = pair - sec * per;             // 0 q, 1 k, 2 v
        r0 = sec * a.inner + (q >> 5) * 64 + (q & 31);
        r1 = r0 + 32;
        return pair < 3 * per;
    } else if (MODE == MODE_GEGLU) {
        const int F = a.N / 2;
        r0 = pair; r1 = pair + F;
        return pair < F;
    } else if (MODE == MODE_LOGITS) {
        const int per = (a.N + 1) / 2;
        sidx = pair / per;
        r0 = 2 * (pair - sidx * per); r1 = r0 + 1;
        return sidx < a.streams;
    }
    r0 = 2 * pair; r1 = r0 + 1;
    return r0 < a.N;
}

// One CHUNK = 1024 consecutive floats of the input vector(s) = PF x 256-float strips; lane l of a wave works on the 4-vectors
// 4 l + 256 i of every row (fixed summation order: lane-strided 4-vectors in ascending k, then the lane tree below).
struct RowChunk { f32x4 pa[PF], pb[PF]; };
struct PairInfo { const float *w0, *w1; int r0, r1, sidx; bool valid, has1; };

template <int MODE>
__device__ __forceinline__ PairInfo pair_info(const GemvArgs& a, int pair)
{
    PairInfo p;
    p.valid = pair_rows<MODE>(a, pair, p.r0, p.r1, p.sidx);
    p.has1 = p.valid && p.r1 < a.N;
    p.w0 = a.W + (int64_t)(p.valid ? p.r0 : 0) * a.ldw;
    p.w1 = a.W + (int64_t)(p.has1 ? p.r1 : (p.valid ? p.r0 : 0)) * a.ldw;
    return p;
}

// chunk c of the two weight rows of a pair: independent of the input vectors, so the HBM / MALL round trip overlaps whatever
// precedes the dot product (the staging of x).  Strips are classified with WAVE-UNIFORM conditions (whole / partial / absent): the
// common whole strip carries no lane masks (a lane-wise guard on every strip cost 290 selects and 220 spilled mask registers).
__device__ __forceinline__ void load_chunk(const GemvArgs& a, const PairInfo& p, int c, int lane, RowChunk& w)
{
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int kb = 1024 * c + 256 * i, k = kb + 4 * lane;
        if (kb + 256 <= a.K) { w.pa[i] = wload4(p.w0 + k); w.pb[i] = wload4(p.w1 + k); }
        else if (kb < a.K) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            w.pa[i] = z; w.pb[i] = z;
            if (k < a.K) { w.pa[i] = wload4(p.w0 + k); w.pb[i] = wload4(p.w1 + k); }
        }
    }
}

// Lane tree: the xor butterfly 32, 16, 8, 4, 2, 1 ("v += shfl_xor(v, o)").  For BQ values per lane it runs as a reduce-scatter - at
// the first log2(BQ) steps a lane keeps half of its values and hands the other half to its partner - which computes, for every value,
// exactly the sums of the plain butterfly (own + partner's, fp addition commutes) with 2 BQ + ... instead of 6 BQ exchanges: the same
// bits for every BQ.  Afterwards value b sits in the lanes with (lane >> (6 - log2 BQ)) == b.
// One reduce-scatter step of the lane tree over H value pairs (v[j], v[j + H]): afterwards lanes with (lane & o) == 0 hold
// v[j][l] + v[j][l ^ o] in v[j], the others v[j + H][l] + v[j + H][l ^ o].  o = 32 / 16: gfx950's v_permlane32_swap / v_permlane16_swap
// exchange the upper half (odd rows) of one register with the lower half (even rows) of the other - one swap and one add per pair, no
// selects, no LDS permute (round-6 first form: two selects + ds_bpermute + add).  o = 8: both sums by DPP row rotation, one select.
template <int H, int N>
__device__ __forceinline__ void tree_step(float (&v)[N], int lane, int o)
{
#pragma unroll
    for (int j = 0; j < H; ++j) {                     // (H is a template constant: v is indexed statically and stays in registers)
        if (o == 32) {
            const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[j]), __float_as_uint(v[j + H]), false, false);
            v[j] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        } else if (o == 16) {
            const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[j]), __float_as_uint(v[j + H]), false, false);
            v[j] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        } else {
            const float t0 = xor_add8(v[j]), t1 = xor_add8(v[j + H]);
            v[j] = (lane & 8) ? t1 : t0;
        }
    }
}
template <int BQ>
__device__ __forceinline__ void lane_tree(float (&v)[BQ], int lane)
{
    if constexpr (BQ == 8) { tree_step<4>(v, lane, 32); tree_step<2>(v, lane, 16); tree_step<1>(v, lane, 8); }
    if constexpr (BQ == 4) { tree_step<2>(v, lane, 32); tree_step<1>(v, lane, 16); }
    if constexpr (BQ == 2) { tree_step<1>(v, lane, 32); }
    // the plain steps that are left (all lanes of a slot's group end up with the total)
    if constexpr (BQ == 1) v[0] += __shfl_xor(v[0], 32, 64);
    if constexpr (BQ <= 2) v[0] += __shfl_xor(v[0], 16, 64);
    if constexpr (BQ <= 4) v[0] = xor_add8(v[0]);
    v[0] = xor_add4(v[0]);
    v[0] = xor_add2(v[0]);
    v[0] = xor_add1(v[0]);
}
template <int BQ> struct SlotShift { static constexpr int value = BQ == 8 ? 3 : BQ == 4 ? 4 : BQ == 2 ? 5 : 6; };

// LDS image of one chunk of the BQ input vectors.  BQ >= 2: slots interleaved in pairs, xs[(b >> 1)][k][b & 1], so that the two
// slots of a pair sit in one 64-bit register pair and a v_pk_fma_f32 advances both (two independent fp32 FMAs: the bits of fmaf).
template <int BQ>
__device__ __forceinline__ void stage_chunk(const GemvArgs& a, int bofs, int c, int Kin, float* xs, float (&ss)[BQ])
{
    const int k = 1024 * c + 4 * (int)threadIdx.x;
    const float* const xg = a.x + (int64_t)bofs * a.x_stride + k;
    const bool in = k < Kin;                          // (Kin is a multiple of 4; wave-uniform whenever it is a multiple of 256)
    f32x4 gk = {1.f, 1.f, 1.f, 1.f};
    if (in && a.gamma) gk = aload4(a.gamma + k);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};             // zero padding of the last chunk: a partial strip multiplies it with zero weights
    const int t4 = 4 * (int)threadIdx.x;
    if (BQ == 1) {
        const f32x4 v = in ? aload4(xg) : z;
#pragma unroll
        for (int e = 0; e < 4; ++e) ss[0] = fmaf(v[e], v[e], ss[0]);
        *reinterpret_cast<f32x4*>(xs + t4) = v * gk;
    } else {
        // HB slots per pass: their 16-byte loads are independent (one L2 round trip per pass), then slot pair by slot pair with a
        // scheduling barrier in between - left alone the scheduler keeps the raw values, the products and the interleaved copies of all
        // eight slots live at once (96 registers on top of the weight strips: two blocks per CU).  (BQ = 8 staged in two passes of
        // four slots: 152 -> 144 registers only - still three blocks per CU - for a second round trip.)
        constexpr int HB = BQ;
#pragma unroll
        for (int h = 0; h < BQ / HB; ++h) {
            f32x4 v[HB];
#pragma unroll
            for (int b = 0; b < HB; ++b) v[b] = in ? aload4(xg + (int64_t)(h * HB + b) * a.x_stride) : z;
#pragma unroll
            for (int q = 0; q < HB / 2; ++q) {
                const int bp = h * (HB / 2) + q;
                const f32x4 va = v[2 * q], vb = v[2 * q + 1];
#pragma unroll
                for (int e = 0; e < 4; ++e) { ss[2 * bp] = fmaf(va[e], va[e], ss[2 * bp]); ss[2 * bp + 1] = fmaf(vb[e], vb[e], ss[2 * bp + 1]); }
                const f32x4 pa = va * gk, pb = vb * gk;
                const f32x4 lo = {pa[0], pb[0], pa[1], pb[1]};
                const f32x4 hi = {pa[2], pb[2], pa[3], pb[3]};
                float* const d = xs + ((size_t)bp * 1024 + t4) * 2;
                *reinterpret_cast<f32x4*>(d) = lo;
                *reinterpret_cast<f32x4*>(d + 4) = hi;
                if (BQ >= 4) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// accumulators of one output row over the BQ slots of a group: slot pairs as 64-bit register pairs (v_pk_fma_f32 operands)
template <int BQ> struct Acc {
    f32x2 p[(BQ + 1) / 2];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < (BQ + 1) / 2; ++i) p[i] = f32x2{0.f, 0.f};
    }
    __device__ __forceinline__ void unpack(float (&v)[BQ]) const {
#pragma unroll
        for (int b = 0; b < BQ; ++b) v[b] = p[b >> 1][b & 1];
    }
};

// one 256-float strip of a row pair against the staged vectors of the BQ slots
template <int BQ>
__device__ __forceinline__ void dot_strip(const float* xs, int xk, const f32x4 a0, const f32x4 a1, Acc<BQ>& acc0, Acc<BQ>& acc1)
{
    if (BQ == 1) {
        const f32x4 xw = *reinterpret_cast<const f32x4*>(xs + xk);
#pragma unroll
        for (int e = 0; e < 4; ++e) { acc0.p[0][0] = fmaf(a0[e], xw[e], acc0.p[0][0]); acc1.p[0][0] = fmaf(a1[e], xw[e], acc1.p[0][0]); }
    } else {
#pragma unroll
        for (int bp = 0; bp < BQ / 2; ++bp) {
            const float* const sp = xs + ((size_t)bp * 1024 + xk) * 2;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(sp), hi = *reinterpret_cast<const f32x4*>(sp + 4);
            const f32x2 xe[4] = {{lo[0], lo[1]}, {lo[2], lo[3]}, {hi[0], hi[1]}, {hi[2], hi[3]}};
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc0.p[bp] = fma2(splat2(a0[e]), xe[e], acc0.p[bp]); acc1.p[bp] = fma2(splat2(a1[e]), xe[e], acc1.p[bp]); }
        }
    }
}

// dot products of one row pair with one staged chunk: acc0 row 0, acc1 row 1 (strips past K are skipped wave-uniformly; inside a
// partial strip the lanes past K multiply zero weights with the zero padding stage_chunk wrote)
template <int BQ>
__device__ __forceinline__ void dot_chunk(const GemvArgs& a, int c, int xoff, const float* xs, const RowChunk& w, int lane,
                                          Acc<BQ>& acc0, Acc<BQ>& acc1)
{
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        if (1024 * c + 256 * i < a.K) dot_strip<BQ>(xs, xoff + 4 * lane + 256 * i, w.pa[i], w.pb[i], acc0, acc1);
    }
}

// the MODE epilogue of one (row pair, slot): s0 / s1 = the two rows' finished dot products
template <int MODE>
__device__ __forceinline__ void gemv_epilogue(const GemvArgs& a, const PairInfo& p, int slot, float s0, float s1)
{
    float* const yb = a.y + (int64_t)slot * a.y_stride;
    const int r0 = p.r0, r1 = p.r1;
    if (a.bias) { s0 += a.bias[r0]; if (p.has1) s1 += a.bias[r1]; }
    if (MODE == MODE_QKV) {
        // every slot decodes at its own position (continuous batching: slots are refilled at different steps)
        const int pos = min(aloadi(a.state + SR * slot), a.max_len - 1);
        const int sec = r0 / a.inner, c0 = r0 - sec * a.inner;        // column inside q / k / v
        if (sec < 2) {                                                // half-split RoPE on the (i, i+32) pair
            const float c = a.rope_cos[pos * 32 + (c0 & 31)], s = a.rope_sin[pos * 32 + (c0 & 31)];
            const float n0 = s0 * c - s1 * s, n1 = s1 * c + s0 * s;
            s0 = n0; s1 = n1;
        }
        float* dst = sec == 0 ? yb : (sec == 1 ? a.k_cache : a.v_cache) + slot * a.cache_stride + (int64_t)pos * a.inner;
        dst[c0] = s0;
        dst[c0 + 32] = s1;
    } else if (MODE == MODE_RES) {
        yb[r0] = aload(yb + r0) + s0;
        if (p.has1) yb[r1] = aload(yb + r1) + s1;
    } else if (MODE == MODE_GEGLU) {
        yb[r0] = s0 * gelu_erf(s1);                                   // F.gelu(gate) * x, text2semantic.py:154-157
    } else if (MODE == MODE_LOGITS) {
        yb[p.sidx * a.N + r0] = s0;
        if (p.has1) yb[p.sidx * a.N + r1] = s1;
    } else {
        yb[r0] = s0;
        if (p.has1) yb[r1] = s1;
    }
}

// y[slot] = epilogue(W . norm(x[slot])) for the slots of the block's groups.  PPW = row pairs per wave (the wave's weight strips stay in
// registers for every group of slots it walks); BQ = slots per group.  The input vectors go through LDS in chunks of 1024 floats (32
// KiB at BQ = 8: four blocks per CU whatever K is), staged with ONE 16-byte load per thread and slot - the launch is one link of a
// chain of 34 dependent launches per token, and its critical path is [weight strip | x chunk] -> FMAs -> lane tree -> store.
// (Round 5 staged scalar-wise, four dependent L2 round trips per 1024 floats, ran the lane tree once per value - 96 exchanges per
// pair at BQ = 8 against 20 now - and left the epilogue of all slots to lane 0.)  Per-(row, slot) arithmetic does not depend on BQ, PPW
// or the grouping: same bits.
// Only PPW = 1, LOOP = false is built (one row pair per wave, one slot group per block: see cvx_t2s_decode_steps).  The two parameters
// stay because folding them into the body changes the compiler's schedule of that kernel.
template <int MODE, int BQ, int PPW = 1, bool LOOP = false>
__global__ __launch_bounds__(256) void gemv_kernel(const GemvArgs a)
{
    __shared__ __attribute__((aligned(16))) float xs[BQ * 1024];
    __shared__ float red[BQ][4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int Kin = (MODE == MODE_LOGITS) ? a.K * a.streams : a.K;     // staged length per slot
    const int nchunk = (Kin + 1023) >> 10;
    // block -> (row block, first slot group).  More than one block per row block (gy > 1): the gy blocks of a row block are
    // consecutive ON ONE XCD (blocks are dealt to the 8 XCDs round robin), so the first one brings the rows into that XCD's L2
    int rb = blockIdx.x, g0 = 0;
    if (a.gy > 1) {
        const int xcd = blockIdx.x & 7, i = blockIdx.x >> 3;
        rb = (i / a.gy) * 8 + xcd;
        g0 = (i % a.gy) * a.gl;
        if (rb >= a.n_blocks) return;                                   // (block-uniform)
    }
    PairInfo pi[PPW];
    RowChunk w[PPW];                                                    // the current chunk of the wave's weight rows (K <= 1024: all of them,
#pragma unroll                                                          // loaded once for every group of slots the block walks)
    for (int p = 0; p < PPW; ++p) pi[p] = pair_info<MODE>(a, (rb * 4 + wid) * PPW + p);
    load_chunk(a, pi[0], 0, lane, w[0]);                                // weights first: in flight under the staging of x
    // (the strips of a second row pair are requested BEHIND the staging, in flight under the first pair's dot products: 32 registers
    //  fewer across the staging - 204 -> 170 VGPRs at two pairs per wave; with the group loop a template constant, 152 -> 118 at one)
    constexpr int SH = SlotShift<BQ>::value;
    const int myb = BQ == 1 ? 0 : lane >> SH;                          // the slot (of a group) whose results the lane tree leaves here
    const bool writer = (lane & ((1 << SH) - 1)) == 0;
    // LOOP: the block walks a.gl groups of slots with its weight strips in registers; the shipped form is ONE group per block - no loop, so nothing (the second pair's strips in particular) has to stay live across a back edge
    const int n_g = LOOP ? a.gl : 1;
#pragma unroll 1
    for (int g = 0; g < n_g; ++g) {
        const int bofs = (g0 + g) * BQ;
        Acc<BQ> acc0[PPW], acc1[PPW];
        float ss[BQ];
#pragma unroll
        for (int b = 0; b < BQ; ++b) ss[b] = 0.f;
#pragma unroll
        for (int p = 0; p < PPW; ++p) { acc0[p].zero(); acc1[p].zero(); }
#pragma unroll 1
        for (int c = 0; c < nchunk; ++c) {
            const bool reload = c > 0 || (g > 0 && nchunk > 1);
            if (reload) load_chunk(a, pi[0], c, lane, w[0]);
            if (g | c) __syncthreads();                                 // (xs / red of the previous chunk / group are free)
            stage_chunk<BQ>(a, bofs, c, Kin, xs, ss);
            __syncthreads();
            if (PPW > 1 && (reload || (g | c) == 0)) {
#pragma unroll
                for (int p = 1; p < PPW; ++p) load_chunk(a, pi[p], c, lane, w[p]);
            }
#pragma unroll
            for (int p = 0; p < PPW; ++p) {
                // LOGITS: the staged vector holds `streams` slices; the pair's slice starts at sidx * K (one chunk: Kin <= 1024)
                const int xoff = (MODE == MODE_LOGITS) ? pi[p].sidx * a.K : 0;
                dot_chunk<BQ>(a, c, xoff, xs, w[p], lane, acc0[p], acc1[p]);
            }
        }
        float inv = 1.f;
        if (a.gamma) {                                                  // F.normalize(eps = 1e-12) * sqrt(dim)
            lane_tree<BQ>(ss, lane);
            if (writer) red[myb][wid] = ss[0];
            __syncthreads();
            const float tot = red[myb][0] + red[myb][1] + red[myb][2] + red[myb][3];
            inv = sqrtf((float)Kin) / fmaxf(sqrtf(tot), 1e-12f);
        }
#pragma unroll
        for (int p = 0; p < PPW; ++p) {
            if (!pi[p].valid) {
                if (MODE == MODE_GEGLU) {      // zero the K padding of the consumer GEMV
                    const int pair = (rb * 4 + wid) * PPW + p;
                    if (pair >= a.N / 2 && pair < a.y_pad && lane < BQ) a.y[(int64_t)(bofs + lane) * a.y_stride + pair] = 0.f;
                }
                continue;
            }
            float v0[BQ], v1[BQ];
            acc0[p].unpack(v0);
            acc1[p].unpack(v1);
            lane_tree<BQ>(v0, lane);
            lane_tree<BQ>(v1, lane);
            if (writer) gemv_epilogue<MODE>(a, pi[p], bofs + myb, v0[0] * inv, v1[0] * inv);
        }
    }
}

// ---------------------------------------------------------------- attention of ONE query over n cached keys
struct AttnArgs {
    const float* q;          // [batch][heads*64]
    const float* k;          // key j of head h at k + B*batch_stride + j*stride + h*64; B = the slot (self-attention cache) or the
    const float* v;          // dialogue the slot is decoding (cross-attention context, n_fixed == -2 / by_dialogue)
    int64_t stride, batch_stride;
    float* out;              // [batch][heads*64]
    const int* state;        // [batch][SR]
    int n_fixed;             // >= 0: that many keys; -1: state[slot][0] + 1 (self-attention); -2: state[slot][3] (context length)
    int by_dialogue;         // 1: k / v are per DIALOGUE (state[slot][4]), not per slot
    float scale;
    int max_len;
};

// sc: T2S_MAX_KEYS floats, red: 4 floats, part: 16 x 64 floats (16-byte aligned) of LDS; all 256 threads of the block
// IND (self-attention of the beam chain): key / value j come from the cache of slot own[j], own = the slot's row of the ancestry table
// owner[2][batch][max_len] (row ((pos & 1) * batch + b)), staged in LDS (own: T2S_MAX_KEYS ints) with one load per thread and 256 keys - a
// key is still ONE global round trip and four stay in flight; loop shape, arithmetic and accumulation order are those of the direct form:
// an identity table gives the same bits.
template <bool IND = false>
__device__ __forceinline__ void attn_body(const AttnArgs& a, int h, int b, int heads, float* sc, float* red, float (*part)[64],
                                          const int* owner = nullptr, int* own = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int HD64 = heads * 64;
    // an idle slot (position max_len: a drained dialogue queue, or a slot past its last step) has nothing to attend to - without
    // this exit it would walk max_len stale cache rows every step (block-uniform)
    if (a.n_fixed < 0 && aloadi(a.state + SR * b) >= a.max_len) return;
    const int n = a.n_fixed >= 0 ? a.n_fixed
                                 : (a.n_fixed == -1 ? min(aloadi(a.state + SR * b) + 1, a.max_len) : min(aloadi(a.state + SR * b + 3), T2S_MAX_KEYS));
    const int64_t kvb = a.by_dialogue ? aloadi(a.state + SR * b + 4) : b;
    const float* const kb = a.k + kvb * a.batch_stride;
    const float* const vb = a.v + kvb * a.batch_stride;
    if constexpr (IND) {
        const int nbat = (int)gridDim.y;                   // (an entry outside [0, batch) is clamped: a stray table stays inside the caches)
        const int* const orow = owner + ((int64_t)(aloadi(a.state + SR * b) & 1) * nbat + b) * a.max_len;
        for (int j = tid; j < n; j += 256) own[j] = min(max(aloadi(orow + j), 0), nbat - 1);
        __syncthreads();
    }
    const int sub = tid & 15, grp = tid >> 4;              // 16 lanes per key, 16 keys per pass
    const f32x4 q4 = aload4(a.q + (int64_t)b * HD64 + h * 64 + 4 * sub);
    float mx = -3.0e38f;
    // four key rows per thread in flight (the loop is a chain of cache round trips otherwise: one 16-byte load, four shuffles and a
    // compare per trip - 38 dependent trips at 600 keys); the arithmetic per key is unchanged
    for (int j0 = 0; j0 < n; j0 += 64) {
        f32x4 k4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 16 * u + grp;
            if constexpr (IND) { if (j < n) k4[u] = aload4(a.k + own[j] * a.batch_stride + (int64_t)j * a.stride + h * 64 + 4 * sub); }
            else if (j < n) k4[u] = aload4(kb + (int64_t)j * a.stride + h * 64 + 4 * sub);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 16 * u + grp;
            float d = 0.f;
            if (j < n) d = k4[u][0] * q4[0] + k4[u][1] * q4[1] + k4[u][2] * q4[2] + k4[u][3] * q4[3];
            d = xor_add1(xor_add2(xor_add4(xor_add8(d))));              // the 16 lanes of a key (xor 8, 4, 2, 1: no LDS permute)
            d *= a.scale;
            if (j < n) { if (sub == 0) sc[j] = d; mx = fmaxf(mx, d); }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mx), 0x128, 0xF, 0xF, false)));
    mx = fmaxf(mx, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(mx), 0x101F)));
    mx = fmaxf(mx, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mx), 0x4E, 0xF, 0xF, false)));
    mx = fmaxf(mx, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mx), 0xB1, 0xF, 0xF, false)));
    if (lane == 0) red[wid] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int j = tid; j < n; j += 256) { const float p = expf(sc[j] - mx); sc[j] = p; sum += p; }
    sum = wave_sum(sum);
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    sum = red[0] + red[1] + red[2] + red[3];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = grp; j0 < n; j0 += 64) {              // (value rows four at a time; accumulated in ascending key order as before)
        f32x4 v4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if constexpr (IND) { if (j0 + 16 * u < n) v4[u] = aload4(a.v + own[j0 + 16 * u] * a.batch_stride + (int64_t)(j0 + 16 * u) * a.stride + h * 64 + 4 * sub); }
            else if (j0 + 16 * u < n) v4[u] = aload4(vb + (int64_t)(j0 + 16 * u) * a.stride + h * 64 + 4 * sub);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (j0 + 16 * u < n) {
                const float p = sc[j0 + 16 * u];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(p, v4[u][e], acc[e]);
            }
        }
    }
    *reinterpret_cast<f32x4*>(&part[grp][4 * sub]) = acc;
    __syncthreads();
    if (tid < 64) {
        float o = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) o += part[g][tid];
        a.out[(int64_t)b * HD64 + h * 64 + tid] = o / sum;
    }
}

__global__ __launch_bounds__(256) void attn_kernel(const AttnArgs a)
{
    __shared__ float sc[T2S_MAX_KEYS];
    __shared__ float red[4];
    __shared__ __attribute__((aligned(16))) float part[16][64];
    attn_body(a, blockIdx.x, blockIdx.y, gridDim.x, sc, red, part);
}

// self-attention of the beam chain: keys and values through the ancestry table
__global__ __launch_bounds__(256) void attn_owner_kernel(const AttnArgs a, const int* owner)
{
    __shared__ float sc[T2S_MAX_KEYS];
    __shared__ int own[T2S_MAX_KEYS];
    __shared__ float red[4];
    __shared__ __attribute__((aligned(16))) float part[16][64];
    attn_body<true>(a, blockIdx.x, blockIdx.y, gridDim.x, sc, red, part, owner, own);
}

// ---------------------------------------------------------------- logit filter + Gumbel argmax, eos bookkeeping, next input
struct SampleArgs {
    const float* logits;     // [batch][streams, V]
    const float* uniforms;   // [dialogue][uniform_steps][streams, V]
    const float* emb;        // [V, dim_emb]
    float* x;                // [batch][streams * dim_emb]  next step's input (residual stream)
    int64_t* tokens;         // [dialogue][streams, max_len]
    int* state;              // [batch][SR]: [0] pos  [1] done  [2] length at the first eos  [3] context rows  [4] dialogue  [5] step limit
                             //              [6] flags (bit 0: the eos does not end the dialogue; bit 1, LOGP instantiations only: FORCED - the
                             //              token row already holds the tokens, nothing is sampled, only the step limit ends the dialogue)
    int* queue;              // NULL, or {next pending dialogue, number of dialogues}: continuous batching
    int* dialogues;          // [n][SR] (queue != NULL): in [0] context rows [1] step limit [2] flags; out [3] status (0 pending, 1 running,
                             //   2 ended by its eos, 3 by its limit) [4] steps decoded [5] the slot it ran in
    const float* start;      // [streams * dim_emb] start token (queue != NULL): the input of a refilled slot
    int batch, uniform_steps;
    int V, dim_emb, streams, max_len, top_k, eos_id;
    float inv_temp;
    float cfg_scale;         // > 1: classifier-free guidance (text2semantic.py:780-792) - slots 2u (text context) and 2u + 1 (context
                             // masked out: the learned null key / value only) decode the SAME tokens: slot 2u samples from
                             // null + (cond - null) * cfg_scale and feeds both; one-output models.  With a queue the pair decodes the
                             // dialogue records (2u', 2u' + 1) and the even slot refills both
    float top_p;             // FILT_TOP_P: the nucleus threshold
    float* logprobs;         // LOGP instantiations: [dialogue][streams, max_len], laid out like tokens
};

enum { FILT_TOP_K = CVX_T2S_FILTER_TOP_K, FILT_TOP_P = CVX_T2S_FILTER_TOP_P };

// One row of logits -> one token: filter (text2semantic.py:118-132), then argmax of kept / temperature + Gumbel noise from the row's
// uniform draws (:105-113).  lrow: the logits; nrow: NULL, or the null-context logits of a guided pair (the filter then acts on
// null + (cond - null) * cfg_scale).  NT threads (a multiple of 64, <= 1024); every thread owns the vocabulary entries tid, tid + NT, ...
// The kept set and the token are exact functions of the logits, the threshold and the uniforms, so they do not depend on NT, the slot,
// the batch or the neighbouring slots:
//   FILT_TOP_K  rank counting (entry i is kept iff fewer than top_k logits are larger: any order gives the same count);
//   FILT_TOP_P  entry i is kept iff the softmax mass of the entries sorted before it is <= top_p (F.pad(cum_probs > thres, (1, -1)),
//               :120-122).  "Sorted before" = a larger logit, or an equal logit at a LOWER INDEX (torch.sort leaves the order of ties
//               open; this is the stable descending order).  The mass is summed per entry over ex[j] = exp(l_j - max) in ascending j
//               (adding 0 for the entries that do not count), and compared with top_p times the sum of all ex[j] in ascending j - the
//               same additions in the same order whoever computes them.  The largest entry has mass 0 before it and is always kept.
// then argmax with the lowest index on ties.  KEEP: also write the kept mask (the stand-alone entry point).
// lg: 1024 floats, ex: 1024 floats (FILT_TOP_P only), bv / bi: 16 entries, chosen: one int of LDS.  Returns the token (block-uniform);
// the caller synchronises before it calls again.
template <int NT, int FILT, bool KEEP>
__device__ __forceinline__ int sample_select(const float* lrow, const float* nrow, float cfg_scale, const float* urow, int V, int top_k,
                                             float top_p, float inv_temp, uint8_t* keep, float* lg, float* ex, float* bv, int* bi, int* chosen)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int i = tid; i < V; i += NT) {
        const float c = aload(lrow + i);
        if (nrow) {             // null_logits + (logits - null_logits) * cond_scale, the reference's operation order (no contraction here)
            const float n = aload(nrow + i);
            lg[i] = n + (c - n) * cfg_scale;
        } else lg[i] = c;
    }
    if (tid < 4 && V + tid < ((V + 3) & ~3)) lg[V + tid] = -INFINITY;      // (the loops below read whole 4-vectors)
    __syncthreads();
    if (FILT == FILT_TOP_P) {
        float m = -INFINITY;
        for (int i = tid; i < V; i += NT) m = fmaxf(m, lg[i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (lane == 0) bv[wid] = m;
        __syncthreads();
        m = bv[0];
        for (int w = 1; w < NT / 64; ++w) m = fmaxf(m, bv[w]);             // (a maximum: exact in any order)
        for (int i = tid; i < ((V + 3) & ~3); i += NT) ex[i] = i < V ? expf(lg[i] - m) : 0.f;
        __syncthreads();                                                   // (bv is written again below)
    }
    float val = -INFINITY;
    int idx = tid;
    for (int i = tid; i < V; i += NT) {
        const float me = lg[i];
        bool kept;
        if (FILT == FILT_TOP_P) {
            float before = 0.f, tot = 0.f;
            for (int j = 0; j < V; j += 4) {
                const f32x4 l4 = *reinterpret_cast<const f32x4*>(lg + j);
                const f32x4 e4 = *reinterpret_cast<const f32x4*>(ex + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool bf = l4[e] > me || (l4[e] == me && j + e < i);
                    before += bf ? e4[e] : 0.f;
                    tot += e4[e];
                }
            }
            kept = before <= top_p * tot;
        } else {
            int cnt = 0;
            for (int j = 0; j < V; j += 4) {         // rank of entry i = number of larger logits (exact: any order gives the same count)
                const f32x4 l4 = *reinterpret_cast<const f32x4*>(lg + j);
                cnt += (l4[0] > me ? 1 : 0) + (l4[1] > me ? 1 : 0) + (l4[2] > me ? 1 : 0) + (l4[3] > me ? 1 : 0);
            }
            kept = cnt < top_k;
        }
        if (KEEP) keep[i] = kept ? 1 : 0;
        if (kept) {
            const float u = urow[i];
            const float g = -logf(fmaxf(-logf(fmaxf(u, 1e-20f)), 1e-20f));
            const float v = me * inv_temp + g;
            if (v > val) { val = v; idx = i; }       // (ascending i: the lowest index wins ties)
        }
    }
    // argmax, lowest index on ties (torch.argmax)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(val, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
    }
    if (lane == 0) { bv[wid] = val; bi[wid] = idx; }
    __syncthreads();
    if (tid == 0) {
        float best = bv[0]; int bt = bi[0];
        for (int w = 1; w < NT / 64; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < bt)) { best = bv[w]; bt = bi[w]; }
        *chosen = bt;
    }
    __syncthreads();
    return *chosen;
}

// The row the filter sees, alone (a forced step, the stand-alone log-prob entry): the loads and the guidance combination of sample_select,
// the same operations in the same order, so lg holds the same bits.  lg: 1024 floats of LDS; synchronises before it returns.
template <int NT>
__device__ __forceinline__ void stage_row(const float* lrow, const float* nrow, float cfg_scale, int V, float* lg)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < V; i += NT) {
        const float c = aload(lrow + i);
        if (nrow) {
            const float n = aload(nrow + i);
            lg[i] = n + (c - n) * cfg_scale;
        } else lg[i] = c;
    }
    __syncthreads();
}

// The maximum m of the staged row lg[0, V) (every thread; exact in any order) and sum_j expf(lg[j] - m) (the threads of the first wave).
// The sum is a function of the row alone - whatever NT, the slot, the batch or the launch: ex[j] = expf(lg[j] - m) for j < V and 0
// up to 1024; lane t of the first wave adds ex[t], ex[t + 64], ..., ex[t + 960] in that order, then the xor butterfly 32, 16, 8, 4, 2, 1
// over the 64 lanes.  lg: the row (as sample_select / stage_row left it, already synchronised), ex: 1024 floats, bv: 16 floats of LDS.
// The ONE definition behind cvx_t2s_logprob_f32, the scoring epilogue and the beam shortlist, which promise each other the same bits.
// The caller synchronises before lg, ex or bv are written again.
template <int NT>
__device__ __forceinline__ float row_expsum(const float* lg, int V, float* ex, float* bv, float& m)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    m = -INFINITY;
    for (int i = tid; i < V; i += NT) m = fmaxf(m, lg[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) bv[wid] = m;
    __syncthreads();
    m = bv[0];
    for (int w = 1; w < NT / 64; ++w) m = fmaxf(m, bv[w]);
    for (int i = tid; i < 1024; i += NT) ex[i] = i < V ? expf(lg[i] - m) : 0.f;
    __syncthreads();
    float sum = 0.f;
    if (tid < 64) {
#pragma unroll
        for (int i = 0; i < 16; ++i) sum += ex[tid + 64 * i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    }
    return sum;
}

// log-softmax of the staged row at entry tok: lp = (lg[tok] - m) - logf(sum), valid in thread 0
template <int NT>
__device__ __forceinline__ float row_logprob(const float* lg, int V, int tok, float* ex, float* bv)
{
    float m;
    const float sum = row_expsum<NT>(lg, V, ex, bv, m);
    return threadIdx.x < 64 ? (lg[tok] - m) - logf(sum) : 0.f;
}

// ---- history rules (cvx_t2s_decode_steps_rules, cvx_t2s_rules_f32; the definition: include/covomix_hip.h): what an output stream has
// emitted so far - its own token row at positions [0, pos), a forced prefix included - changes the row the filter sees, in this order:
// repetition penalty, no-repeat n-gram, minimum length.  Part of the SELECTION, like the filter: log-probs stay those of the unmodified row.
struct RulesArgs {
    const int* table;        // [n_records][RULES_WORDS] 32-bit words: [0] float theta [1] int window [2] int ngram [3] int min_len
    int n_records;
};
constexpr int RULES_WORDS = 4;
constexpr int RULES_MAX_NGRAM = 8;
struct Rules { float theta; int W, n, m; };

// a table row with stray values clamped (they index nothing either way): n into [0, 8], W and m into [0, cap], theta <= 0 or NaN -> 1 (off)
__device__ __forceinline__ Rules rules_row(const int* row, int cap)
{
    Rules r;
    r.theta = __int_as_float(row[0]);
    if (!(r.theta > 0.f)) r.theta = 1.f;
    r.W = min(max(row[1], 0), cap);
    r.n = min(max(row[2], 0), RULES_MAX_NGRAM);
    r.m = min(max(row[3], 0), cap);
    return r;
}

// Per-id marks of the history h[0, pos) in LDS (pen, ban: 1024 bytes each; two arrays of bytes, every store writes a 1: no read-modify-write):
//   pen[t]  t occurs in h[max(0, pos - W), pos)  (W = 0: in all of h)
//   ban[t]  t = h[e] for a position e in [n - 1, pos) whose n - 1 predecessors equal the last n - 1 tokens of h (n = 1: every id of h)
// tid strides over the positions; an id outside [0, V) marks nothing.  The history was written by earlier launches on the stream (or by
// the host): plain loads.  Synchronises before it returns.  T: int64_t - a token row in global memory (the sampled chains); int - the
// history a beam hypothesis gathered into LDS along its ancestry (beam_history).
template <int NT, class T = int64_t>
__device__ __forceinline__ void rules_marks(const T* h, int pos, int V, const Rules& r, uint8_t* pen, uint8_t* ban)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < 1024; i += NT) { pen[i] = 0; ban[i] = 0; }
    __syncthreads();
    const int lo = r.W > 0 ? max(0, pos - r.W) : 0;
    const int n1 = r.n - 1;
    for (int e = tid; e < pos; e += NT) {
        const T t = h[e];
        if (t < 0 || t >= V) continue;
        if (e >= lo) pen[t] = 1;
        if (r.n >= 1 && e >= n1) {
            bool same = true;
            for (int i = 0; i < n1; ++i) same = same && h[e - n1 + i] == h[pos - n1 + i];
            if (same) ban[t] = 1;
        }
    }
    __syncthreads();
}

// entry i of the row the filter sees under the rules: stage_row's value, the penalty (an IEEE division), the eos below the minimum length, the ban
__device__ __forceinline__ float rules_value(const float* lrow, const float* nrow, float cfg_scale, int i, float theta, bool pen, bool no_eos, bool ban)
{
    float l = aload(lrow + i);
    if (nrow) {
        const float n = aload(nrow + i);
        l = n + (l - n) * cfg_scale;
    }
    if (pen) l = l > 0.f ? __fdiv_rn(l, theta) : l * theta;
    return (no_eos || ban) ? -INFINITY : l;
}

// stage_row under the rules: lg[0, V) from the marks.  When no entry is finite afterwards the n-gram bans of this step are void: the banned
// entries are staged again without the ban (the penalty and the eos suppression stay).  lg: 1024 floats of LDS; synchronises before it returns.
template <int NT>
__device__ __forceinline__ void rules_stage(const float* lrow, const float* nrow, float cfg_scale, int V, int pos, int eos_id, const Rules& r,
                                            const uint8_t* pen, const uint8_t* ban, float* lg)
{
    const int tid = threadIdx.x;
    int finite = 0;
    for (int i = tid; i < V; i += NT) {
        const float l = rules_value(lrow, nrow, cfg_scale, i, r.theta, pen[i] != 0, i == eos_id && pos < r.m, ban[i] != 0);
        lg[i] = l;
        finite |= (l - l == 0.f) ? 1 : 0;               // (neither an infinity nor a NaN)
    }
    if (!__syncthreads_or(finite)) {                    // (block-uniform)
        for (int i = tid; i < V; i += NT)
            if (ban[i]) lg[i] = rules_value(lrow, nrow, cfg_scale, i, r.theta, pen[i] != 0, i == eos_id && pos < r.m, false);
    }
    __syncthreads();
}

// per-dialogue settings (cvx_t2s_decode_steps_per_dialogue, cvx_t2s_decode_steps_mixed)
struct PerArgs {
    const int* table;        // [n_records][PER_WORDS] 32-bit words: [0] float inv_temp [1] int filter mode [2] int top_k [3] float top_p
                             //                                     [4] float cfg_scale [5] int prefix_len [6], [7] reserved
    int n_records;
};
constexpr int PER_WORDS = 8;

// The slot of the null half beside text half b: b + 1 in the launch-wide pair layout, slot pb in the mixed pool.  Spelled out at every use:
// with b + 1 routed through a variable the compiler schedules the default kernels differently (1,260 -> 1,257 instructions).
template <bool MIXED> __device__ __forceinline__ int null_slot(int b, int pb)
{
    if constexpr (MIXED) return pb;
    else return b + 1;
}

// The sampling step of slot b: ONE body behind sample_kernel, sample_per_kernel and sample_mixed_kernel (NT threads, all of the block).
// Per output stream: the token (sample_select, or read from the token row on a given step), its log-prob (LOGP), the embedding = the next
// input; then the eos bookkeeping and, behind a dialogue queue, the refill.  What the parameters choose:
//   FILT, PER   the SETTINGS.  !PER: temperature, top_k, top_p and the guidance scale from SampleArgs, the filter from FILT.  PER: from the
//               settings row of the DIALOGUE the slot decodes (slot record [4]) - a refilled slot picks up the new dialogue's settings because
//               it now names that dialogue - with the filter chosen at run time (block-uniform: a branch around the two sample_select
//               forms) and a forced prefix: while pos < prefix_len the step is a given step.
//   LOGP        the log-prob epilogue and the FORCED flag (bit 1): every step of such a dialogue is a given step.
//               A GIVEN step reads its token from the dialogue's token row (clamped into [0, V)), reads no uniforms, and its eos ends nothing.
//   MIXED       the PAIRING.  !MIXED: cfg_scale > 1 is the launch's layout - slots (2u, 2u + 1) decode the records (dlg, dlg + 1), the odd
//               block returns at once and the even one feeds both slots and writes the null record's token row too.  MIXED: slot record [7]
//               is the slot's role - 0 single, p + 1 the text half of a pair whose null half is slot p (any slot: partners need not be
//               neighbours), -(p + 1) the null half of slot p, whose block returns at once; the null record's token row is not written
//               (nothing reads it).
//               And the TAIL.  !MIXED: without a queue the slot record moves on; with one, a block that ends its dialogue takes the next
//               pending one.  MIXED: such a block only writes the record(s) and idles its slot(s) - it never touches the queue.  Handing out
//               records is the business of mixed_schedule_kernel, the launch that follows: a guided head needs TWO idle slots, which no
//               single block can know.  That launch clears the null half's role too, not this one: the null half's own block may be reading
//               it now, and with the role unchanged every word a block decides by is its own slot's or constant during the launch (no fences).
//   RULES       (with PER) the HISTORY RULES of the dialogue's row of the rules table, on sampled steps only: the marks of the stream's own
//               token row below pos, the ruled row staged into lg, then sample_select as it is, reading that row from lg (every thread
//               copies its own entries onto themselves).  LOGP: the unmodified row is staged again before the epilogue - the given-step path.
// lg, ex: 1024 floats (ex: FILT_TOP_P, PER or LOGP only), bv / bi: 16 entries, chosen: one int of LDS; pen, ban: 1024 bytes each (RULES only).
template <int NT, int FILT, bool LOGP, bool PER, bool MIXED, bool RULES = false>
__device__ __forceinline__ void sample_step(const SampleArgs& a, const PerArgs& p, int b, float* lg, float* ex, float* bv, int* bi, int* chosen,
                                            const RulesArgs* ru = nullptr, uint8_t* pen = nullptr, uint8_t* ban = nullptr)
{
    static_assert(!RULES || PER, "the rules chain reads its settings per dialogue");
    const int tid = threadIdx.x;
    const bool cfg = !MIXED && a.cfg_scale > 1.0f;
    if (cfg && (b & 1)) return;                     // the null-context slot follows its partner (block-uniform)
    int* const state = a.state + SR * b;
    const int pos = aloadi(state);
    if (pos >= a.max_len) return;                   // (block-uniform) an idle slot: a drained queue, or past its last step
    const int role = MIXED ? aloadi(state + 7) : 0;
    if (MIXED && role < 0) return;                  // the null half follows its partner (block-uniform)
    const bool pair = MIXED ? role > 0 : cfg;
    const int pb = MIXED && pair ? min(a.batch - 1, role - 1) : b;      // (a stray role indexes no slot outside the batch)
    int* const sn = MIXED ? a.state + SR * pb : state + SR;             // the null half's slot record (touched for a pair only)
    const int64_t dlg = aloadi(state + 4);          // the dialogue this slot decodes (== b without a queue)
    // PER: the dialogue's settings (block-uniform: every thread reads the same row).  A stray record number reads row 0 / the last row, and
    // stray values cannot index anything: top_k is clamped into [1, V], an unknown mode is top-k, P is clamped into [0, step limit]
    const int* const row = PER ? p.table + (int64_t)PER_WORDS * min((int64_t)(p.n_records - 1), max((int64_t)0, dlg)) : nullptr;
    const float inv_temp = PER ? __int_as_float(row[0]) : a.inv_temp;
    const bool nucleus = PER ? row[1] == FILT_TOP_P : FILT == FILT_TOP_P;
    const int top_k = PER ? min(a.V, max(1, row[2])) : a.top_k;
    const float top_p = PER ? __int_as_float(row[3]) : a.top_p;
    const float scale = PER ? __int_as_float(row[4]) : a.cfg_scale;
    const int plim = (MIXED || a.queue) ? aloadi(state + 5) : a.max_len;    // (without a queue the slot record's limit is the caller's business)
    const int P = PER ? min(max(plim, 0), max(0, row[5])) : 0;
    // (block-uniform: every thread reads the record.)  !PER: `given` must be the constant-folded `forced` - pos is loaded, so a `pos < 0` that
    // can never hold would stay in the default kernel (1,260 -> 1,319 instructions, another VGPR granule)
    const bool forced = LOGP ? (aloadi(state + 6) & 2) != 0 : false;
    const bool given = PER ? forced || pos < P : forced;
    bool eos = false;
    for (int s = 0; s < a.streams; ++s) {
        const float* const lrow = a.logits + ((int64_t)b * a.streams + s) * a.V;
        const float* const nrow = pair ? a.logits + ((int64_t)null_slot<MIXED>(b, pb) * a.streams + s) * a.V : nullptr;
        int tok;
        if (given) {
            if (LOGP) stage_row<NT>(lrow, nrow, scale, a.V, lg);          // (without the epilogue nothing reads the row)
            // (the host refuses tokens outside [0, V); the clamp keeps a stray one from indexing emb)
            tok = (int)min((int64_t)(a.V - 1), max((int64_t)0, a.tokens[(dlg * a.streams + s) * a.max_len + pos]));
        } else {
            const float* const urow = a.uniforms + ((dlg * a.uniform_steps + pos) * a.streams + s) * a.V;
            if constexpr (RULES) {
                const Rules r = rules_row(ru->table + (int64_t)RULES_WORDS * min((int64_t)(ru->n_records - 1), max((int64_t)0, dlg)), a.max_len);
                rules_marks<NT>(a.tokens + (dlg * a.streams + s) * a.max_len, pos, a.V, r, pen, ban);
                rules_stage<NT>(lrow, nrow, scale, a.V, pos, a.eos_id, r, pen, ban, lg);
                if (nucleus) tok = sample_select<NT, FILT_TOP_P, false>(lg, nullptr, 1.f, urow, a.V, top_k, top_p, inv_temp, nullptr, lg, ex, bv, bi, chosen);
                else tok = sample_select<NT, FILT_TOP_K, false>(lg, nullptr, 1.f, urow, a.V, top_k, top_p, inv_temp, nullptr, lg, ex, bv, bi, chosen);
                if (LOGP) stage_row<NT>(lrow, nrow, scale, a.V, lg);
            } else
            if constexpr (!PER) tok = sample_select<NT, FILT, false>(lrow, nrow, scale, urow, a.V, top_k, top_p, inv_temp, nullptr, lg, ex, bv, bi, chosen);
            else if (nucleus) tok = sample_select<NT, FILT_TOP_P, false>(lrow, nrow, scale, urow, a.V, top_k, top_p, inv_temp, nullptr, lg, ex, bv, bi, chosen);
            else tok = sample_select<NT, FILT_TOP_K, false>(lrow, nrow, scale, urow, a.V, top_k, top_p, inv_temp, nullptr, lg, ex, bv, bi, chosen);
            if (tid == 0) a.tokens[(dlg * a.streams + s) * a.max_len + pos] = tok;
        }
        if (LOGP) {          // of the row the filter saw: before the filter, the temperature and the noise
            const float lp = row_logprob<NT>(lg, a.V, tok, ex, bv);
            if (tid == 0) a.logprobs[(dlg * a.streams + s) * a.max_len + pos] = lp;
        }
        // a given eos ends nothing: PER leaves it out here, !PER in ends_eos below, where given == forced.  (One form for both - all eos here,
        // `&& !given` below - is the same function and moved sample_per_kernel<false> by 9 instructions: the default chain's text is kept.)
        eos = eos || (tok == a.eos_id && !(PER && given));
        for (int d = tid; d < a.dim_emb; d += NT) {
            const float e = a.emb[(int64_t)tok * a.dim_emb + d];
            a.x[((int64_t)b * a.streams + s) * a.dim_emb + d] = e;
            if (pair) a.x[((int64_t)null_slot<MIXED>(b, pb) * a.streams + s) * a.dim_emb + d] = e;
        }
        if (!MIXED && pair && tid == 0) a.tokens[((dlg + 1) * a.streams + s) * a.max_len + pos] = tok;
        __syncthreads();
    }
    if (!MIXED && a.queue == nullptr) {
        if (LOGP && forced) {       // the slot record's step limit ends a forced dialogue: done, its length, and the slot idles
            if (tid == 0) {
                const bool last = pos + 1 >= aloadi(state + 5);
                const int np = last ? a.max_len : pos + 1;
                if (last) { state[1] = 1; state[2] = pos + 1; }
                state[0] = np;
                if (pair) { if (last) { sn[1] = 1; sn[2] = pos + 1; } sn[0] = np; }
            }
            return;
        }
        if (tid == 0) {
            int done = aloadi(state + 1), len = aloadi(state + 2);
            if (eos && done == 0) { done = 1; len = pos + 1; state[1] = 1; state[2] = len; }
            state[0] = pos + 1;
            if (pair) { sn[1] = done; sn[2] = len; sn[0] = pos + 1; }
        }
        return;
    }
    // continuous batching: the dialogue ends with its first eos (text2semantic.py:803-818) or at its step limit; the slot then
    // takes the next pending dialogue: position 0, the start token as input, that dialogue's context / uniforms / token rows.
    // A pair: the text half decides for both; the pair's dialogue records are (dlg, dlg + 1) and the queue hands out two records
    // at a time.  A pair is taken only when BOTH of its records exist (nxt + 1 < n), so a refill never indexes past the n dialogues
    // whatever the caller put into queue[1].
    const bool ends_eos = eos && !(aloadi(state + 6) & 1) && !(!PER && forced);
    const bool ends = ends_eos || pos + 1 >= aloadi(state + 5);        // (block-uniform: `eos` comes from LDS, the record is read by all)
    if (!ends) {
        if (tid == 0) { state[0] = pos + 1; if (pair) sn[0] = pos + 1; }
        return;
    }
    if (tid == 0) {
        int* const dr = a.dialogues + SR * dlg;
        dr[4] = pos + 1;
        dr[5] = b;
        if (pair) { dr[SR + 4] = pos + 1; dr[SR + 5] = null_slot<MIXED>(b, pb); }
        __threadfence();
        dr[3] = ends_eos ? 2 : 3;
        if (pair) dr[SR + 3] = ends_eos ? 2 : 3;
        if constexpr (!MIXED) {
            const int take = pair ? 2 : 1;
            const int nxt = atomicAdd(a.queue, take);
            *chosen = nxt + take - 1 < aloadi(a.queue + 1) ? nxt : -1;
        }
    }
    int nxt = -1;
    if constexpr (!MIXED) { __syncthreads(); nxt = *chosen; }
    if (nxt < 0) {                                  // nothing pending: the slot idles (every kernel clamps / skips at max_len)
        if (tid == 0) {
            state[0] = a.max_len; state[1] = 1;
            if (MIXED) state[7] = 0;                // (sn[7]: mixed_schedule_kernel, above)
            if (pair) { sn[0] = a.max_len; sn[1] = 1; }
        }
        return;
    }
    for (int d = tid; d < a.dim_emb * a.streams; d += NT) {
        const float e = a.start[d];
        a.x[(int64_t)b * a.streams * a.dim_emb + d] = e;
        if (pair) a.x[(int64_t)null_slot<MIXED>(b, pb) * a.streams * a.dim_emb + d] = e;
    }
    if (tid == 0) {
        int* const dn = a.dialogues + SR * nxt;
        state[0] = 0; state[1] = 0; state[2] = 0; state[3] = dn[0]; state[4] = nxt; state[5] = dn[1]; state[6] = dn[2];
        dn[5] = b;
        dn[3] = 1;
        if (pair) {
            sn[0] = 0; sn[1] = 0; sn[2] = 0; sn[3] = dn[SR + 0]; sn[4] = nxt + 1; sn[5] = dn[1]; sn[6] = dn[2];
            dn[SR + 5] = null_slot<MIXED>(b, pb);
            dn[SR + 3] = 1;
        }
    }
}

// FILT_TOP_K is the instruction stream of every default launch; the nucleus filter's second LDS array (exp(l - max), 4 KiB on top of the
// 4 KiB of logits) exists in its own instantiation only
// LOGP (cvx_t2s_decode_steps_scored): the log-prob epilogue and the forced mode, in instantiations of their own
template <int FILT, bool LOGP = false>
__global__ __launch_bounds__(1024) void sample_kernel(const SampleArgs a)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[(FILT == FILT_TOP_P || LOGP) ? 1024 : 4];
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ int chosen;
    sample_step<1024, FILT, LOGP, false, false>(a, PerArgs{nullptr, 0}, blockIdx.x, lg, ex, bv, bi, &chosen);
}

// settings per dialogue and forced prefixes (cvx_t2s_decode_steps_per_dialogue)
template <bool LOGP>
__global__ __launch_bounds__(1024) void sample_per_kernel(const SampleArgs a, const PerArgs p)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ int chosen;
    sample_step<1024, FILT_TOP_K, LOGP, true, false>(a, p, blockIdx.x, lg, ex, bv, bi, &chosen);
}

// guided and unguided dialogues in one slot pool (cvx_t2s_decode_steps_mixed)
template <bool LOGP>
__global__ __launch_bounds__(1024) void sample_mixed_kernel(const SampleArgs a, const PerArgs p)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ int chosen;
    sample_step<1024, FILT_TOP_K, LOGP, true, true>(a, p, blockIdx.x, lg, ex, bv, bi, &chosen);
}

// the per-dialogue and the mixed chain under the history rules (cvx_t2s_decode_steps_rules)
template <bool LOGP>
__global__ __launch_bounds__(1024) void sample_rules_kernel(const SampleArgs a, const PerArgs p, const RulesArgs ru)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ int chosen;
    __shared__ uint8_t pen[1024], ban[1024];
    sample_step<1024, FILT_TOP_K, LOGP, true, false, true>(a, p, blockIdx.x, lg, ex, bv, bi, &chosen, &ru, pen, ban);
}

template <bool LOGP>
__global__ __launch_bounds__(1024) void sample_mixed_rules_kernel(const SampleArgs a, const PerArgs p, const RulesArgs ru)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ int chosen;
    __shared__ uint8_t pen[1024], ban[1024];
    sample_step<1024, FILT_TOP_K, LOGP, true, true, true>(a, p, blockIdx.x, lg, ex, bv, bi, &chosen, &ru, pen, ban);
}

// the history rules alone: one block per row, no slot state (cvx_t2s_rules_f32)
struct RulesRowsArgs {
    const float* logits;     // [rows, V]
    const int64_t* history;  // [rows, hist_ld]
    const int* hist_len;     // [rows]: pos, clamped into [0, hist_ld]
    const int* table;        // [rows][RULES_WORDS]
    float* out;              // [rows, V]
    int V, hist_ld, eos_id;
};

__global__ __launch_bounds__(1024) void rules_rows_kernel(const RulesRowsArgs a)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ uint8_t pen[1024], ban[1024];
    const int64_t r = blockIdx.x;
    const int pos = min(max(a.hist_len[r], 0), a.hist_ld);
    const Rules ru = rules_row(a.table + RULES_WORDS * r, 0x7fffffff);
    rules_marks<1024>(a.history + r * a.hist_ld, pos, a.V, ru, pen, ban);
    rules_stage<1024>(a.logits + r * a.V, nullptr, 1.f, a.V, pos, a.eos_id, ru, pen, ban, lg);
    for (int i = threadIdx.x; i < a.V; i += 1024) a.out[r * a.V + i] = lg[i];
}

// The scheduler of the mixed pool: ONE block, launched after sample_mixed_kernel (the kernel boundary makes every record write of that
// launch visible - no fence, no cross-block traffic).  Serial and deterministic, thread 0 (t2s.py: mixed_schedule replays it on the host):
//   F = the idle slots (record [0] >= max_len) in ascending order; loop: h = queue[0]; stop if h >= queue[1] or F is empty; record h
//   unguided: the lowest slot of F takes it, h += 1; guided (flag bit 2): stop if h + 1 >= queue[1] (never index past the records) or F
//   holds fewer than two slots (the head waits: strict order); else the lowest slot of F becomes the text half of record h, the next one
//   the null half of record h + 1, h += 2.
// Re-arming a slot is sample_step's refill - position 0, [3]..[6] from the record, record [3] = 1 and [5] = the slot - plus the role
// in [7]; all threads then copy `start` into the x rows of the armed slots.  Slots that stay idle get role 0 (the null half of a pair
// that ended in the sampling launch still carries its role).  Plain stores only: nothing else runs beside this block.
__global__ __launch_bounds__(1024) void mixed_schedule_kernel(const SampleArgs a)
{
    __shared__ int armed[T2S_MAX_BATCH];
    __shared__ int n_armed;
    __shared__ unsigned long long left;
    const int tid = threadIdx.x;
    if (tid < 64) {
        const bool idle = tid < a.batch && aloadi(a.state + SR * tid) >= a.max_len;
        unsigned long long F = __ballot(idle);
        if (tid == 0) {
            int h = aloadi(a.queue), cnt = 0;
            const int n = aloadi(a.queue + 1);
            while (F != 0ull && h >= 0 && h < n) {
                int* const dn = a.dialogues + SR * (int64_t)h;
                const int s0 = __ffsll((long long)F) - 1;
                if (!(dn[2] & CVX_T2S_FLAG_GUIDED)) {
                    F &= F - 1ull;
                    int* const st = a.state + SR * s0;
                    st[0] = 0; st[1] = 0; st[2] = 0; st[3] = dn[0]; st[4] = h; st[5] = dn[1]; st[6] = dn[2]; st[7] = 0;
                    dn[5] = s0;
                    dn[3] = 1;
                    armed[cnt++] = s0;
                    h += 1;
                    continue;
                }
                if (h + 1 >= n || (F & (F - 1ull)) == 0ull) break;
                F &= F - 1ull;
                const int s1 = __ffsll((long long)F) - 1;
                F &= F - 1ull;
                int* const st = a.state + SR * s0;
                int* const sn = a.state + SR * s1;
                st[0] = 0; st[1] = 0; st[2] = 0; st[3] = dn[0]; st[4] = h; st[5] = dn[1]; st[6] = dn[2]; st[7] = s1 + 1;
                sn[0] = 0; sn[1] = 0; sn[2] = 0; sn[3] = dn[SR + 0]; sn[4] = h + 1; sn[5] = dn[1]; sn[6] = dn[2]; sn[7] = -(s0 + 1);
                dn[5] = s0;
                dn[3] = 1;
                dn[SR + 5] = s1;
                dn[SR + 3] = 1;
                armed[cnt++] = s0;
                armed[cnt++] = s1;
                h += 2;
            }
            if (cnt > 0) a.queue[0] = h;
            n_armed = cnt;
            left = F;
        }
    }
    __syncthreads();
    if (tid < a.batch && ((left >> tid) & 1ull) && aloadi(a.state + SR * tid + 7) != 0) a.state[SR * tid + 7] = 0;
    const int cnt = n_armed, row = a.dim_emb * a.streams;
    for (int i = tid; i < cnt * row; i += 1024) {
        const int k = i / row, d = i - k * row;
        a.x[(int64_t)armed[k] * row + d] = a.start[d];
    }
}

// the log-prob epilogue alone: one block per row, no slot state (cvx_t2s_logprob_f32)
__global__ __launch_bounds__(1024) void logprob_rows_kernel(const float* logits, const int64_t* tokens, int V, float* out)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    const int64_t r = blockIdx.x;
    stage_row<1024>(logits + r * V, nullptr, 1.f, V, lg);
    const int64_t t = tokens[r];
    const bool in = t >= 0 && t < V;                      // (a token outside [0, V) indexes nothing: its row gets a NaN)
    const float lp = row_logprob<1024>(lg, V, in ? (int)t : 0, ex, bv);
    if (threadIdx.x == 0) out[r] = in ? lp : __int_as_float(0x7fc00000);
}

// the filter + sampling of sample_kernel alone: one block per row, no slot state, no queue, no embedding write
struct SampleRowsArgs {
    const float* logits;     // [rows, V]
    const float* uniforms;   // [rows, V]
    int64_t* tokens;         // [rows]
    uint8_t* kept;           // [rows, V] or NULL
    int V, top_k;
    float top_p, inv_temp;
};

template <int FILT, bool KEEP>
__global__ __launch_bounds__(1024) void sample_rows_kernel(const SampleRowsArgs a)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[FILT == FILT_TOP_P ? 1024 : 4];
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ int chosen;
    const int64_t r = blockIdx.x;
    const int tok = sample_select<1024, FILT, KEEP>(a.logits + r * a.V, nullptr, 1.f, a.uniforms + r * a.V, a.V, a.top_k, a.top_p, a.inv_temp,
                                                    KEEP ? a.kept + r * a.V : nullptr, lg, ex, bv, bi, &chosen);
    if (threadIdx.x == 0) a.tokens[r] = tok;
}

// ---------------------------------------------------------------- beam search: per-row shortlist, per-utterance selection, back-track
// (the algorithm: include/covomix_hip.h, cvx_t2s_beam_steps)
constexpr int BEAM_MAX = 16;

// The K = min(B, V) entries of one row with the largest log-softmax, ordered by (value descending, index ascending): entry i has rank
// #{j: lp[j] > lp[i] or (lp[j] == lp[i] and j < i)} - a total order, so exactly K entries have a rank below K whatever the ties.
// lp[j] = (lg[j] - m) - logf(sum) with row_logprob's m and sum: the same function of the row.  lg: the staged row (stage_row), ex: 1024
// floats, bv: 16 floats, ls: one float of LDS; out_lp / out_tok [K]: LDS or global.  The caller synchronises before lg / ex are written again.
// RULES (cvx_t2s_beam_rules_steps): between the lp pass and the ranking the banned entries of lp become -inf - ban[i] (rules_marks) and,
// with no_eos, entry V - 1.  When that leaves no un-banned entry (one block-uniform count) the marks of ban are void and the eos ban stays.
// The ranking is the same total order, so a shortlist may hold entries of -inf: the merge gives them no candidate.
template <int NT, bool RULES = false>
__device__ __forceinline__ void beam_shortlist(const float* lg, int V, int K, float* ex, float* bv, float* ls, float* out_lp, int* out_tok,
                                               const uint8_t* ban = nullptr, bool no_eos = false)
{
    const int tid = threadIdx.x;
    float m;
    const float sum = row_expsum<NT>(lg, V, ex, bv, m);
    if (tid == 0) *ls = logf(sum);
    __syncthreads();                                   // (the first wave has read ex)
    const float l = *ls;
    for (int i = tid; i < 1024; i += NT) ex[i] = i < V ? (lg[i] - m) - l : -INFINITY;
    __syncthreads();
    if constexpr (RULES) {
        int open = 0;
        for (int i = tid; i < V; i += NT) open |= (ban[i] || (no_eos && i == V - 1)) ? 0 : 1;
        const bool marks = __syncthreads_or(open) != 0;        // (block-uniform) false: the n-gram bans of this step are void
        for (int i = tid; i < V; i += NT)
            if ((marks && ban[i]) || (no_eos && i == V - 1)) ex[i] = -INFINITY;
        __syncthreads();
    }
    for (int i = tid; i < V; i += NT) {
        const float me = ex[i];
        int cnt = 0;
        for (int j = 0; j < V; j += 4) {
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(ex + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) cnt += (l4[e] > me || (l4[e] == me && j + e < i)) ? 1 : 0;
        }
        if (cnt < K) { out_lp[cnt] = me; out_tok[cnt] = i; }
    }
}

// The B best candidates of one utterance.  Candidate q = (p B + a) B + b: hypothesis p continued with entry a of its stream-0 shortlist and
// entry b of its stream-1 shortlist (b = 0 for one stream), score sc[p] + lp0 or sc[p] + (lp0 + lp1) in fp32; a finished p has the single
// candidate q = p B B with its score unchanged; a p with score -inf has none.  Order: score descending, q ascending.  sel[r] = the r-th best
// q, or -1 when fewer than r + 1 candidates exist.  sc / fin [B], sl_lp [B][S][BEAM_MAX]: LDS or global; bv / bi: 16 entries of LDS.
// NT = 1024 threads hold the B^3 <= 4096 candidates four each; B rounds of a block-wide argmax.
// RULES: a shortlist entry of -inf (banned) gives no candidate.
template <int NT, bool RULES = false>
__device__ __forceinline__ void beam_merge(const float* sc, const int* fin, const float* sl_lp, int B, int S, int K, float* bv, int* bi, int* sel)
{
    static_assert(BEAM_MAX * BEAM_MAX * BEAM_MAX <= 4 * NT, "four candidates per thread");
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    constexpr int NONE = 0x7fffffff;
    f32x4 cs = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};       // the thread's candidates q = tid + NT k, and the mask of those still in play
    unsigned ok = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = tid + NT * k;
        const int p = q / (B * B), a = (q / B) % B, b = q % B;
        if (p < B) {
            const float c = sc[p];
            if (c > -INFINITY) {
                if (fin[p]) { if (a == 0 && b == 0) { ok |= 1u << k; cs[k] = c; } }
                else if (a < K && (S == 2 ? b < K : b == 0)) {
                    const float l0 = sl_lp[(p * S) * BEAM_MAX + a];
                    if constexpr (RULES) {
                        const float l1 = S == 2 ? sl_lp[(p * S + 1) * BEAM_MAX + b] : 0.f;
                        if (l0 > -INFINITY && l1 > -INFINITY) { ok |= 1u << k; cs[k] = S == 2 ? c + (l0 + l1) : c + l0; }
                    } else {
                        ok |= 1u << k;
                        cs[k] = S == 2 ? c + (l0 + sl_lp[(p * S + 1) * BEAM_MAX + b]) : c + l0;
                    }
                }
            }
        }
    }
    for (int r = 0; r < B; ++r) {
        float v = -INFINITY;
        int q = NONE;
#pragma unroll
        for (int k = 0; k < 4; ++k)                    // (ascending q: the lowest wins ties)
            if (((ok >> k) & 1u) && (q == NONE || cs[k] > v)) { v = cs[k]; q = tid + NT * k; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oq = __shfl_xor(q, o, 64);
            if (oq != NONE && (q == NONE || ov > v || (ov == v && oq < q))) { v = ov; q = oq; }
        }
        if (lane == 0) { bv[wid] = v; bi[wid] = q; }
        __syncthreads();
        v = bv[0]; q = bi[0];
        for (int w = 1; w < NT / 64; ++w) {
            const float ov = bv[w];
            const int oq = bi[w];
            if (oq != NONE && (q == NONE || ov > v || (ov == v && oq < q))) { v = ov; q = oq; }
        }
        if (q != NONE && (q % NT) == tid) ok &= ~(1u << (q / NT));
        if (tid == 0) sel[r] = q == NONE ? -1 : q;
        __syncthreads();
    }
}

// what new hypothesis i is, from its candidate q (thread-local; sl_*: the shortlists beam_merge saw)
struct BeamPick { int parent, tok0, tok1; float lp0, lp1, score; int fin; };      // (scalars: an array indexed by the stream leaves the registers)
__device__ __forceinline__ BeamPick beam_pick(int q, int i, const float* sc, const int* fin, const float* sl_lp, const int* sl_tok, int B, int S,
                                              int eos_id)
{
    BeamPick r;
    r.parent = i; r.tok0 = r.tok1 = -1; r.lp0 = r.lp1 = 0.f; r.score = -INFINITY; r.fin = 1;               // no candidate left: a dead slot
    if (q < 0) return r;
    const int p = q / (B * B), a = (q / B) % B, b = q % B;
    r.parent = p;
    r.score = sc[p];
    if (fin[p]) return r;                                                                                  // carried: nothing new
    r.tok0 = sl_tok[(p * S) * BEAM_MAX + a];
    r.lp0 = sl_lp[(p * S) * BEAM_MAX + a];
    if (S == 2) {
        r.tok1 = sl_tok[(p * S + 1) * BEAM_MAX + b];
        r.lp1 = sl_lp[(p * S + 1) * BEAM_MAX + b];
        r.score = r.score + (r.lp0 + r.lp1);
    } else r.score = r.score + r.lp0;
    r.fin = (r.tok0 == eos_id || (S == 2 && r.tok1 == eos_id)) ? 1 : 0;
    return r;
}

// the selection step alone (cvx_t2s_beam_select_f32): one block per group of B hypotheses, its B * S rows one after the other
struct BeamSelectArgs {
    const float* logits;     // [G * B, S, V]
    const float* scores_in;  // [G * B]
    const uint8_t* finished_in;
    int B, S, V;
    int32_t* parents;        // [G * B] (index inside the group)
    int64_t* tokens;         // [G * B, S]
    float* token_lp;         // [G * B, S]
    float* scores_out;
    uint8_t* finished_out;
};

// what cvx_t2s_beam_select_rules_f32 adds: every hypothesis' history given outright, one rules row per group
struct BeamSelectRulesArgs {
    const int* history;      // [G * B][S][hist_ld]
    const int* hist_len;     // [G * B]: pos, clamped into [0, hist_ld]
    const int* table;        // [G][RULES_WORDS]
    int hist_ld;
};

// The ban marks of one row of a beam hypothesis (RULES shortlists): h [pos] = its history, already in LDS.  Without an n-gram rule nothing
// of h is read (pos 0: the marks are cleared only).  Returns whether the eos is banned at this position.
__device__ __forceinline__ bool beam_marks(const int* h, int pos, int V, const Rules& r, uint8_t* pen, uint8_t* ban)
{
    Rules nb = r;
    nb.theta = 1.f; nb.W = 0;                          // (beam search has no repetition penalty: pen is scratch)
    rules_marks<1024, int>(h, r.n >= 1 ? pos : 0, V, nb, pen, ban);
    return pos < r.m;
}

template <bool RULES>
__device__ __forceinline__ void beam_select_step(const BeamSelectArgs& a, const BeamSelectRulesArgs& ra)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ float ls;
    __shared__ float sl_lp[BEAM_MAX * 2 * BEAM_MAX];
    __shared__ int sl_tok[BEAM_MAX * 2 * BEAM_MAX];
    __shared__ float sc[BEAM_MAX];
    __shared__ int fin[BEAM_MAX];
    __shared__ int sel[BEAM_MAX];
    const int tid = threadIdx.x, B = a.B, S = a.S;
    const int64_t base = (int64_t)blockIdx.x * B;
    const int K = min(B, a.V);
    if (tid < B) { sc[tid] = a.scores_in[base + tid]; fin[tid] = a.finished_in[base + tid] ? 1 : 0; }
    __syncthreads();
    for (int row = 0; row < B * S; ++row) {
        const int p = row / S;
        if (fin[p] || !(sc[p] > -INFINITY)) continue;                  // (block-uniform) no candidates from this row
        stage_row<1024>(a.logits + (base * S + row) * a.V, nullptr, 1.f, a.V, lg);
        if constexpr (RULES) {
            __shared__ int hrow[T2S_MAX_KEYS];
            __shared__ uint8_t pen[1024], ban[1024];
            const int pos = min(max(ra.hist_len[base + p], 0), ra.hist_ld);
            const Rules r = rules_row(ra.table + RULES_WORDS * (int64_t)blockIdx.x, 0x7fffffff);
            if (r.n >= 1)
                for (int j = tid; j < pos; j += 1024) hrow[j] = ra.history[(base * S + row) * (int64_t)ra.hist_ld + j];     // (base: int64_t)
            __syncthreads();
            const bool no_eos = beam_marks(hrow, pos, a.V, r, pen, ban);
            beam_shortlist<1024, true>(lg, a.V, K, ex, bv, &ls, sl_lp + row * BEAM_MAX, sl_tok + row * BEAM_MAX, ban, no_eos);
        } else
            beam_shortlist<1024>(lg, a.V, K, ex, bv, &ls, sl_lp + row * BEAM_MAX, sl_tok + row * BEAM_MAX);
        __syncthreads();
    }
    beam_merge<1024, RULES>(sc, fin, sl_lp, B, S, K, bv, bi, sel);
    if (tid < B) {
        const BeamPick r = beam_pick(sel[tid], tid, sc, fin, sl_lp, sl_tok, B, S, a.V - 1);
        a.parents[base + tid] = r.parent;
        a.tokens[(base + tid) * S] = r.tok0; a.token_lp[(base + tid) * S] = r.lp0;
        if (S == 2) { a.tokens[(base + tid) * S + 1] = r.tok1; a.token_lp[(base + tid) * S + 1] = r.lp1; }
        a.scores_out[base + tid] = r.score;
        a.finished_out[base + tid] = (uint8_t)r.fin;
    }
}

__global__ __launch_bounds__(1024) void beam_select_kernel(const BeamSelectArgs a) { beam_select_step<false>(a, BeamSelectRulesArgs{}); }
__global__ __launch_bounds__(1024) void beam_select_rules_kernel(const BeamSelectArgs a, const BeamSelectRulesArgs ra) { beam_select_step<true>(a, ra); }

// the beam chain's selection: beam_shortlist_kernel (one block per live row) then beam_merge_kernel (one block per utterance)
struct BeamArgs {
    const float* logits;     // [batch][streams, V]
    const float* emb;
    float* x;
    int* state;              // slot records: [0] position (max_len: a finished hypothesis or an ended utterance), [1] finished, [2] its steps
    float* scores;           // [batch]
    uint8_t* finished;       // [batch]
    int* owner;              // [2][batch][max_len]
    int* groups;             // [batch / B][4]: [0] steps done [1] ended [2] step limit
    int* parents;            // [max_len][batch] (index inside the group)
    int* hist_tok;           // [max_len][batch][streams]
    float* hist_lp;
    float* short_lp;         // [batch][streams][BEAM_MAX]
    int* short_tok;
    int64_t* tokens;         // [batch][streams][max_len] (back-track)
    float* logprobs;
    int batch, B, V, dim_emb, streams, max_len;
};

__global__ __launch_bounds__(1024) void beam_shortlist_kernel(const BeamArgs a)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    __shared__ float ls;
    const int row = blockIdx.x, slot = row / a.streams;
    if (aloadi(a.state + SR * slot) >= a.max_len) return;             // (block-uniform) finished, ended or idle: no candidates from this row
    stage_row<1024>(a.logits + (int64_t)row * a.V, nullptr, 1.f, a.V, lg);
    beam_shortlist<1024>(lg, a.V, min(a.B, a.V), ex, bv, &ls, a.short_lp + row * BEAM_MAX, a.short_tok + row * BEAM_MAX);
}

// The shortlist of a GUIDED hypothesis (cvx_t2s_beam_guided_steps): one block per hypothesis h = slots 2h (text context) and 2h + 1 (null
// context); the row is stage_row's null + (cond - null) * scale - the row the guided scoring path takes its log-probs from - and the
// shortlist is kept by hypothesis.  (BeamArgs.batch counts HYPOTHESES in the guided chain: half the slots.)
__global__ __launch_bounds__(1024) void beam_shortlist_guided_kernel(const BeamArgs a, const float scale)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    __shared__ float ls;
    const int h = blockIdx.x;
    if (aloadi(a.state + SR * (2 * h)) >= a.max_len) return;          // (block-uniform) finished, ended or idle: both halves idle together
    stage_row<1024>(a.logits + (int64_t)(2 * h) * a.V, a.logits + (int64_t)(2 * h + 1) * a.V, scale, a.V, lg);
    beam_shortlist<1024>(lg, a.V, min(a.B, a.V), ex, bv, &ls, a.short_lp + h * BEAM_MAX, a.short_tok + h * BEAM_MAX);
}

// what the QUEUE forms of the merge and the back-track need beyond BeamArgs (cvx_t2s_beam_queue_steps: beam search through continuously
// refilled groups); a second kernel argument, as attn_owner_kernel's table
struct BeamQueueArgs {
    int* queue;              // {next pending utterance, number of utterances}
    int* utterances;         // [n][SR]: in [0] context rows [1] step limit; out [3] status [4] steps decoded [5] the group it ran in
    const float* start;      // [streams * dim_emb] start token: the input of every slot of a re-armed group
    int* parents;            // [n][max_len][B] - history by UTTERANCE (a group decodes several, one after the other)
    int* hist_tok;           // [n][max_len][B][streams]
    float* hist_lp;
    float* final_scores;     // [n][B]: scores / steps / finished flags of the B hypotheses when the utterance ended
    int* final_steps;
    uint8_t* final_fin;
    int64_t* tokens;         // [n * B][streams][max_len] (back-track)
    float* logprobs;
    int n, ctx_rows;         // (n: the back-track's thread count; the merge reads queue[1])
};

// where step t of hypothesis i is kept: by slot ([max_len][batch], group g's slots start at g B), or by utterance g ([n][max_len][B])
template <bool QUEUE> __device__ __forceinline__ int64_t beam_hist_index(const BeamArgs& a, int g, int t, int i)
{
    return QUEUE ? ((int64_t)g * a.max_len + t) * a.B + i : (int64_t)t * a.batch + g * a.B + i;
}

// The shortlists under the history rules (cvx_t2s_beam_rules_steps): beam_shortlist_kernel / beam_shortlist_guided_kernel with the bans of
// the hypothesis' OWN history between the lp pass and the ranking.  The history is not one row: it runs through the ancestry table.  At
// position pos the hypothesis' ancestry row own = owner[pos & 1][slot] names in own[j + 1] the slot its ancestor sat in after step j - the
// slot whose new hypothesis the merge of step j recorded in hist_tokens - so
//   h_s[j] = hist_tokens[beam_hist_index(g, j, own[j + 1] / P - base)][s],  j in [0, pos)
// (P slots per hypothesis: the text half's row in the guided chain), two dependent loads per position, strided over the block into LDS.
// beam_merge_step wrote own[0..pos] (the parent's row, then the slot itself) and every named history entry in earlier launches: plain loads.
// A re-armed group sits at position 0: an empty history.  The rules row: the group (lock-step) or its utterance (QUEUE), n and m alone.
// hyp: the hypothesis (== the slot in the unguided chain); returns false for a row without candidates (block-uniform).
template <bool QUEUE, int P>
__device__ __forceinline__ bool beam_history(const BeamArgs& a, const BeamQueueArgs& qa, const RulesArgs& ru, int hyp, int s, int* hrow,
                                             uint8_t* pen, uint8_t* ban, bool& no_eos)
{
    const int tid = threadIdx.x, B = a.B, S = a.streams;
    const int slot = hyp * P;
    const int pos = aloadi(a.state + SR * slot);
    if (pos >= a.max_len || pos < 0) return false;                    // finished, ended or idle
    const int u = hyp / B, base = u * B;
    const int hg = QUEUE ? min(max(aloadi(a.groups + 4 * u + 3), 0), max(aloadi(qa.queue + 1) - 1, 0)) : u;
    const Rules r = rules_row(ru.table + (int64_t)RULES_WORDS * min(ru.n_records - 1, hg), a.max_len);
    if (r.n >= 1) {
        const int* const own = a.owner + ((int64_t)(pos & 1) * a.batch * P + slot) * a.max_len;
        const int* const hist_tok = QUEUE ? qa.hist_tok : a.hist_tok;
        for (int j = tid; j < pos; j += 1024) {                       // (j + 1 <= pos < max_len)
            const int i = min(max(aloadi(own + j + 1) / P - base, 0), B - 1);      // (a stray entry stays inside the group)
            hrow[j] = hist_tok[beam_hist_index<QUEUE>(a, hg, j, i) * S + s];
        }
    }
    __syncthreads();
    no_eos = beam_marks(hrow, pos, a.V, r, pen, ban);
    return true;
}

template <bool QUEUE>
__global__ __launch_bounds__(1024) void beam_shortlist_rules_kernel(const BeamArgs a, const BeamQueueArgs qa, const RulesArgs ru)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    __shared__ float ls;
    __shared__ int hrow[T2S_MAX_KEYS];
    __shared__ uint8_t pen[1024], ban[1024];
    const int row = blockIdx.x, slot = row / a.streams;
    bool no_eos;
    if (!beam_history<QUEUE, 1>(a, qa, ru, slot, row - slot * a.streams, hrow, pen, ban, no_eos)) return;
    stage_row<1024>(a.logits + (int64_t)row * a.V, nullptr, 1.f, a.V, lg);
    beam_shortlist<1024, true>(lg, a.V, min(a.B, a.V), ex, bv, &ls, a.short_lp + row * BEAM_MAX, a.short_tok + row * BEAM_MAX, ban, no_eos);
}

template <bool QUEUE>
__global__ __launch_bounds__(1024) void beam_shortlist_guided_rules_kernel(const BeamArgs a, const BeamQueueArgs qa, const RulesArgs ru,
                                                                          const float scale)
{
    __shared__ __attribute__((aligned(16))) float lg[1024];
    __shared__ __attribute__((aligned(16))) float ex[1024];
    __shared__ float bv[16];
    __shared__ float ls;
    __shared__ int hrow[T2S_MAX_KEYS];
    __shared__ uint8_t pen[1024], ban[1024];
    const int h = blockIdx.x;
    bool no_eos;
    if (!beam_history<QUEUE, 2>(a, qa, ru, h, 0, hrow, pen, ban, no_eos)) return;
    stage_row<1024>(a.logits + (int64_t)(2 * h) * a.V, a.logits + (int64_t)(2 * h + 1) * a.V, scale, a.V, lg);
    beam_shortlist<1024, true>(lg, a.V, min(a.B, a.V), ex, bv, &ls, a.short_lp + h * BEAM_MAX, a.short_tok + h * BEAM_MAX, ban, no_eos);
}

// One selection step of group u = blockIdx.x (1024 threads): the B best candidates, their back-pointers into the history, the scores and
// slot records, then the next inputs and the next ancestry rows.  ONE body behind beam_merge_kernel and beam_merge_queue_kernel.  QUEUE: the
// history is indexed by the group's utterance (group record [3]) and, when the utterance ends, the same launch writes its finals, status and
// steps, takes the next pending one from the queue (one atomicAdd) and re-arms the whole group at position 0; with none left the group ends
// as without a queue.
// GUIDED (cvx_t2s_beam_guided_steps): a hypothesis is a slot PAIR - hypothesis h in slots 2h (text context) and 2h + 1 (null context) - with
// one score, one flag and one history entry; a.batch counts hypotheses, one stream.  Whatever is kept by SLOT is written for both halves:
// the slot records, the next input (the same embedding row) and the ancestry rows (the text row continues the parent's text row, the null
// row the parent's null row).  A re-armed group gives the text half the utterance's context rows and kv_c row 2 * utterance, the null half one
// context row (the learned null key / value) and kv_c row 2 * utterance + 1.
// RULES (cvx_t2s_beam_rules_steps): the shortlists may hold banned entries (-inf), which give no candidate (beam_merge<.., RULES>); a new
// slot left without one is a dead hypothesis as before.  Nothing else differs: the history the rules read is what this body records anyway.
template <bool QUEUE, bool GUIDED = false, bool RULES = false>
__device__ __forceinline__ void beam_merge_step(const BeamArgs& a, const BeamQueueArgs& qa)
{
    constexpr int P = GUIDED ? 2 : 1;                   // slots per hypothesis
    __shared__ float bv[16];
    __shared__ int bi[16];
    __shared__ float sc[BEAM_MAX];
    __shared__ int fin[BEAM_MAX], len[BEAM_MAX], sel[BEAM_MAX];
    __shared__ int n_par[BEAM_MAX], n_fin[BEAM_MAX], n_tok[BEAM_MAX][2];
    const int tid = threadIdx.x, B = a.B, S = a.streams;
    const int u = blockIdx.x, base = u * B;
    int* const gs = a.groups + 4 * u;
    const int t = aloadi(gs);
    // (a refilled group's limit comes from an utterance record: at least one step)
    const int lim = QUEUE ? min(max(aloadi(gs + 2), 1), a.max_len) : min(aloadi(gs + 2), a.max_len);
    if (aloadi(gs + 1) != 0 || t < 0 || t >= lim) return;                  // (block-uniform) ended or idle, or nothing to decode
    // the history's first index: the group, or its utterance (a stray record stays inside the n utterances)
    const int hg = QUEUE ? min(max(aloadi(gs + 3), 0), max(aloadi(qa.queue + 1) - 1, 0)) : u;
    if (tid < B) {
        sc[tid] = a.scores[base + tid];
        fin[tid] = a.finished[base + tid] ? 1 : 0;
        len[tid] = aloadi(a.state + SR * (base + tid) * P + 2);
    }
    __syncthreads();
    const float* const sl_lp = a.short_lp + (int64_t)base * S * BEAM_MAX;
    const int* const sl_tok = a.short_tok + (int64_t)base * S * BEAM_MAX;
    beam_merge<1024, RULES>(sc, fin, sl_lp, B, S, min(B, a.V), bv, bi, sel);
    BeamPick r;
    if (tid < B) {
        r = beam_pick(sel[tid], tid, sc, fin, sl_lp, sl_tok, B, S, a.V - 1);
        const int64_t h = beam_hist_index<QUEUE>(a, hg, t, tid);
        int* const parents = QUEUE ? qa.parents : a.parents;
        int* const hist_tok = QUEUE ? qa.hist_tok : a.hist_tok;
        float* const hist_lp = QUEUE ? qa.hist_lp : a.hist_lp;
        parents[h] = r.parent;
        hist_tok[h * S] = r.tok0; hist_lp[h * S] = r.lp0;
        if (S == 2) { hist_tok[h * S + 1] = r.tok1; hist_lp[h * S + 1] = r.lp1; }
        n_par[tid] = r.parent; n_fin[tid] = r.fin; n_tok[tid][0] = r.tok0; n_tok[tid][1] = r.tok1;
    }
    __syncthreads();                                    // (every old score / flag / length has been read)
    bool all_fin = true;
    for (int i = 0; i < B; ++i) all_fin = all_fin && n_fin[i] != 0;
    const bool ends = all_fin || t + 1 >= lim;
    // a finished hypothesis keeps the steps it took; at the end of the utterance the others took all t + 1
    int steps = 0;
    if (tid < B) steps = r.fin ? (sel[tid] >= 0 && fin[r.parent] ? len[r.parent] : (sel[tid] >= 0 ? t + 1 : 0)) : (ends ? t + 1 : 0);
    if constexpr (QUEUE) {
        if (ends) {                                     // the utterance's finals, status and steps; then the next pending one
            __shared__ int chosen;
            if (tid < B) {
                const int64_t f = (int64_t)hg * B + tid;
                qa.final_scores[f] = r.score;
                qa.final_steps[f] = steps;
                qa.final_fin[f] = (uint8_t)r.fin;
            }
            if (tid == 0) {
                int* const ur = qa.utterances + SR * hg;
                ur[4] = t + 1;
                ur[5] = u;
                __threadfence();
                ur[3] = all_fin ? 2 : 3;
                const int nxt = atomicAdd(qa.queue, 1);
                chosen = nxt >= 0 && nxt < aloadi(qa.queue + 1) ? nxt : -1;
            }
            __syncthreads();
            const int nxt = chosen;
            if (nxt >= 0) {
                // re-arm the group on utterance nxt: position 0, the start token, hypothesis 0 alone live.  The cache and owner rows of the
                // ended utterance stay where they are: the new one's owner rows name only positions it has written itself
                int* const un = qa.utterances + SR * nxt;
                for (int idx = tid; idx < B * P * S * a.dim_emb; idx += 1024)
                    a.x[(int64_t)base * P * S * a.dim_emb + idx] = qa.start[idx % (S * a.dim_emb)];
                if (tid < B) {
                    const int slot = (base + tid) * P;              // (GUIDED: the text half; base + tid is the hypothesis)
                    int* const st = a.state + SR * slot;
                    a.scores[base + tid] = tid == 0 ? 0.f : -__builtin_inff();
                    a.finished[base + tid] = 0;
                    st[0] = 0; st[1] = 0; st[2] = 0; st[3] = min(max(aloadi(un), 1), qa.ctx_rows); st[4] = nxt * P;
                    a.owner[(int64_t)slot * a.max_len] = slot;      // (parity 0, position 0)
                    if constexpr (GUIDED) {
                        st[SR] = 0; st[SR + 1] = 0; st[SR + 2] = 0; st[SR + 3] = 1; st[SR + 4] = nxt * 2 + 1;
                        a.owner[(int64_t)(slot + 1) * a.max_len] = slot + 1;
                    }
                }
                if (tid == 0) {
                    gs[0] = 0; gs[1] = 0; gs[2] = min(max(aloadi(un + 1), 1), a.max_len); gs[3] = nxt;
                    un[5] = u;
                    un[3] = 1;
                }
                return;
            }
        }
    }
    if (tid < B) {
        const int slot = (base + tid) * P;                  // (GUIDED: the text half; base + tid is the hypothesis)
        int* const st = a.state + SR * slot;
        a.scores[base + tid] = r.score;
        a.finished[base + tid] = (uint8_t)r.fin;
        // the slots of an ended utterance idle at max_len, as a finished hypothesis does (the attention kernel's idle exit)
        st[0] = (r.fin || ends) ? a.max_len : t + 1;
        st[1] = (r.fin || ends) ? 1 : 0;
        st[2] = steps;
        if constexpr (GUIDED) {
            st[SR] = (r.fin || ends) ? a.max_len : t + 1;
            st[SR + 1] = (r.fin || ends) ? 1 : 0;
            st[SR + 2] = steps;
        }
    }
    if (tid == 0) { gs[0] = t + 1; if (ends) gs[1] = 1; }
    if (ends) return;
    // the next input of every live hypothesis, and its row of the ancestry table: the parent's row for positions 0..t, then itself
    if constexpr (GUIDED) {
        // (one stream: row r of the group's 2 B slots belongs to hypothesis r / 2; both halves take the same embedding row)
        for (int idx = tid; idx < B * 2 * a.dim_emb; idx += 1024) {
            const int r2 = idx / a.dim_emb, d = idx - r2 * a.dim_emb, i = r2 >> 1;
            if (!n_fin[i]) a.x[((int64_t)base * 2 + r2) * a.dim_emb + d] = a.emb[(int64_t)n_tok[i][0] * a.dim_emb + d];
        }
    } else {
        for (int idx = tid; idx < B * S * a.dim_emb; idx += 1024) {
            const int i = idx / (S * a.dim_emb), rem = idx - i * (S * a.dim_emb), s = rem / a.dim_emb, d = rem - s * a.dim_emb;
            if (!n_fin[i]) a.x[((int64_t)(base + i) * S + s) * a.dim_emb + d] = a.emb[(int64_t)n_tok[i][s] * a.dim_emb + d];
        }
    }
    const int* const src = a.owner + (int64_t)(t & 1) * a.batch * P * a.max_len;
    int* const dst = a.owner + (int64_t)((t + 1) & 1) * a.batch * P * a.max_len;
    for (int i = 0; i < B; ++i) {
        if (n_fin[i]) continue;
#pragma unroll
        for (int half = 0; half < P; ++half) {
            const int* const sr = src + (int64_t)((base + n_par[i]) * P + half) * a.max_len;
            int* const dr = dst + (int64_t)((base + i) * P + half) * a.max_len;
            for (int j = tid; j <= t; j += 1024) dr[j] = aloadi(sr + j);
            if (tid == 0) dr[t + 1] = (base + i) * P + half;     // (t + 1 < max_len: the utterance has not ended)
        }
    }
}

__global__ __launch_bounds__(1024) void beam_merge_kernel(const BeamArgs a) { beam_merge_step<false>(a, BeamQueueArgs{}); }
__global__ __launch_bounds__(1024) void beam_merge_queue_kernel(const BeamArgs a, const BeamQueueArgs qa) { beam_merge_step<true>(a, qa); }
__global__ __launch_bounds__(1024) void beam_merge_guided_kernel(const BeamArgs a) { beam_merge_step<false, true>(a, BeamQueueArgs{}); }
__global__ __launch_bounds__(1024) void beam_merge_guided_queue_kernel(const BeamArgs a, const BeamQueueArgs qa) { beam_merge_step<true, true>(a, qa); }
__global__ __launch_bounds__(1024) void beam_merge_rules_kernel(const BeamArgs a) { beam_merge_step<false, false, true>(a, BeamQueueArgs{}); }
__global__ __launch_bounds__(1024) void beam_merge_queue_rules_kernel(const BeamArgs a, const BeamQueueArgs qa) { beam_merge_step<true, false, true>(a, qa); }
__global__ __launch_bounds__(1024) void beam_merge_guided_rules_kernel(const BeamArgs a) { beam_merge_step<false, true, true>(a, BeamQueueArgs{}); }
__global__ __launch_bounds__(1024) void beam_merge_guided_queue_rules_kernel(const BeamArgs a, const BeamQueueArgs qa) { beam_merge_step<true, true, true>(a, qa); }

// tokens / logprobs [row][streams][max_len] from the back-pointers: one thread per row walks its ancestry.  A row is a slot of group g
// (steps: group record [0]) or, with QUEUE, hypothesis row - g B of utterance g (steps: utterance record [4])
template <bool QUEUE>
__device__ __forceinline__ void beam_backtrack_step(const BeamArgs& a, const BeamQueueArgs& qa)
{
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= (QUEUE ? qa.n * a.B : a.batch)) return;
    const int g = row / a.B, S = a.streams;
    const int T = min(max(aloadi(QUEUE ? qa.utterances + SR * g + 4 : a.groups + 4 * g), 0), a.max_len);
    const int* const parents = QUEUE ? qa.parents : a.parents;
    const int* const hist_tok = QUEUE ? qa.hist_tok : a.hist_tok;
    const float* const hist_lp = QUEUE ? qa.hist_lp : a.hist_lp;
    int64_t* const tokens = QUEUE ? qa.tokens : a.tokens;
    float* const logprobs = QUEUE ? qa.logprobs : a.logprobs;
    int cur = row - g * a.B;
    for (int t = T - 1; t >= 0; --t) {
        const int64_t h = beam_hist_index<QUEUE>(a, g, t, cur);
        for (int s = 0; s < S; ++s) {
            tokens[((int64_t)row * S + s) * a.max_len + t] = hist_tok[h * S + s];
            logprobs[((int64_t)row * S + s) * a.max_len + t] = hist_lp[h * S + s];
        }
        cur = min(max(aloadi(parents + h), 0), a.B - 1);
    }
}

__global__ __launch_bounds__(64) void beam_backtrack_kernel(const BeamArgs a) { beam_backtrack_step<false>(a, BeamQueueArgs{}); }
__global__ __launch_bounds__(64) void beam_backtrack_queue_kernel(const BeamArgs a, const BeamQueueArgs qa) { beam_backtrack_step<true>(a, qa); }

__global__ __launch_bounds__(256) void geglu_kernel(const float* __restrict__ h, float* __restrict__ out, int64_t rows,
                                                   int F, int64_t ld_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * ld_out) return;
    const int64_t r = i / ld_out;
    const int c = (int)(i - r * ld_out);
    out[i] = c < F ? h[r * 2 * F + c] * gelu_erf(h[r * 2 * F + F + c]) : 0.f;
}


// batch 1 / 2 / 4 / 8: one group of that many slots; above: ceil(batch / 8) groups of 8, one block per (row block, group) (the
// per-slot buffers of the caller hold whole groups; the slots past `batch` compute on whatever they hold and nothing reads them)
template <int MODE, int BQ>
void launch_gemv_b(GemvArgs g, int pairs, int groups, hipStream_t st)
{
    g.n_blocks = (pairs + 3) / 4;
    g.gl = 1;
    g.gy = groups;
    const unsigned grid = g.gy > 1 ? (unsigned)((g.n_blocks + 7) / 8 * 8 * g.gy) : (unsigned)g.n_blocks;
    hipLaunchKernelGGL((gemv_kernel<MODE, BQ>), dim3(grid), dim3(256), 0, st, g);
}
template <int MODE>
void launch_gemv(const GemvArgs& g, int pairs, int batch, hipStream_t st)
{
    if (batch <= 1) launch_gemv_b<MODE, 1>(g, pairs, 1, st);
    else if (batch <= 2) launch_gemv_b<MODE, 2>(g, pairs, 1, st);
    else if (batch <= 4) launch_gemv_b<MODE, 4>(g, pairs, 1, st);
    else launch_gemv_b<MODE, 8>(g, pairs, (batch + 7) / 8, st);
}

}  // namespace

extern "C" int cvx_geglu_f32(const float* h, float* out, int64_t rows, int32_t F, int64_t ld_out, cvx_stream_t s)
{
    CVX_REQUIRE(h && out && rows >= 0 && F > 0 && ld_out >= F, "geglu: bad arguments");
    if (rows == 0) return CVX_OK;
    const int64_t n = rows * ld_out;
    hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cvx_hip_stream(s),
                       h, out, rows, F, ld_out);
    CVX_CHECK_LAUNCH("cvx_geglu_f32");
    return CVX_OK;
}

// the filter settings of the decode and of cvx_t2s_sample_f32: top-k needs 1 <= k <= V, top-p a threshold inside (0, 1)
static int t2s_filter_validate(int32_t mode, int32_t k, float thres, int32_t V)
{
    CVX_REQUIRE(mode == CVX_T2S_FILTER_TOP_K || mode == CVX_T2S_FILTER_TOP_P, "t2s: unknown filter mode %d", mode);
    CVX_REQUIRE(mode != CVX_T2S_FILTER_TOP_K || (k >= 1 && k <= V), "t2s: top_k = %d outside [1, vocab = %d]", k, V);
    CVX_REQUIRE(mode != CVX_T2S_FILTER_TOP_P || (thres > 0.f && thres < 1.f), "t2s: top_p = %g outside (0, 1)", (double)thres);
    return CVX_OK;
}

extern "C" int cvx_t2s_sample_f32(const float* logits, const float* uniforms, int64_t rows, int32_t V, int32_t filter_mode, int32_t k,
                                  float thres, float temperature, int64_t* tokens, uint8_t* kept, cvx_stream_t s)
{
    CVX_REQUIRE(logits && uniforms && tokens && rows >= 0 && rows <= 0x7fffffff && V > 0 && V <= 1024 && temperature >= 0.f,
                "t2s_sample: bad arguments (rows=%lld V=%d)", (long long)rows, V);
    const int frc = t2s_filter_validate(filter_mode, k, thres, V);
    if (frc != CVX_OK) return frc;
    if (rows == 0) return CVX_OK;
    const SampleRowsArgs a{logits, uniforms, tokens, kept, V, k, thres, 1.0f / fmaxf(temperature, 1e-10f)};
    const dim3 grid((unsigned)rows), block(1024);
    hipStream_t st = cvx_hip_stream(s);
    if (filter_mode == CVX_T2S_FILTER_TOP_P) {
        if (kept) hipLaunchKernelGGL((sample_rows_kernel<FILT_TOP_P, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((sample_rows_kernel<FILT_TOP_P, false>), grid, block, 0, st, a);
    } else {
        if (kept) hipLaunchKernelGGL((sample_rows_kernel<FILT_TOP_K, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((sample_rows_kernel<FILT_TOP_K, false>), grid, block, 0, st, a);
    }
    CVX_CHECK_LAUNCH("cvx_t2s_sample_f32");
    return CVX_OK;
}

// per_dialogue (cvx_t2s_decode_steps_per_dialogue): the sampling scalars of the descriptor are ignored and need not be valid
static int t2s_validate(const cvx_t2s_decoder* d, int32_t n_steps, bool per_dialogue = false)
{
    CVX_REQUIRE(d && d->layers && n_steps >= 0, "t2s_decode: null decoder");
    CVX_REQUIRE(d->dim > 0 && d->dim % 4 == 0 && d->dim <= T2S_MAX_DIM && d->inner == d->heads * 64 && d->depth > 0 &&
                d->streams >= 1 && d->streams <= 2 && d->dim_emb * d->streams == d->dim && d->dim_emb % 4 == 0 &&
                (d->streams == 1 || d->dim <= 1024) && d->vocab > 0 && d->vocab <= 1024 &&
                d->ff_inner > 0 && d->ff_inner_pad >= d->ff_inner && d->ff_inner_pad % 4 == 0 && d->ff_inner_pad <= T2S_MAX_DIM &&
                d->n_ctx >= 0 && d->n_ctx <= T2S_MAX_KEYS && d->max_len > 0 && d->max_len <= T2S_MAX_KEYS &&
                (per_dialogue || d->temperature >= 0.f) && d->batch >= 1 && d->batch <= T2S_MAX_BATCH &&
                d->uniform_steps > 0 &&
                d->ctx_rows > 0 && d->ctx_rows <= T2S_MAX_KEYS && d->n_ctx <= d->ctx_rows,
                "t2s_decode: bad dimensions (dim=%d inner=%d heads=%d streams=%d dim_emb=%d vocab=%d ff=%d/%d n_ctx=%d/%d max_len=%d batch=%d)",
                d->dim, d->inner, d->heads, d->streams, d->dim_emb, d->vocab, d->ff_inner, d->ff_inner_pad, d->n_ctx, d->ctx_rows,
                d->max_len, d->batch);
    CVX_REQUIRE(!(d->cfg_scale > 1.f) || (d->streams == 1 && d->batch % 2 == 0 && d->n_ctx == 0),
                "t2s_decode: guidance (cfg_scale > 1) needs a one-output model, an even batch (context / null-context slot pairs) and "
                "per-slot context rows (n_ctx == 0)");
    CVX_REQUIRE(!d->queue || (d->dialogues && d->start && d->n_ctx == 0),
                "t2s_decode: a dialogue queue needs the dialogue records, the start token and per-dialogue context rows (n_ctx == 0)");
    CVX_REQUIRE(!(d->queue && d->cfg_scale > 1.f) || (d->n_dialogues > 0 && d->n_dialogues % 2 == 0),
                "t2s_decode: a dialogue queue under guidance holds record PAIRS (text context, null context): n_dialogues = %d must be "
                "the even, positive number of records", d->n_dialogues);
    CVX_REQUIRE(d->n_dialogues >= 0, "t2s_decode: n_dialogues = %d", d->n_dialogues);
    if (!per_dialogue) {
        const int frc = t2s_filter_validate(d->filter_mode, d->top_k, d->top_p, d->vocab);
        if (frc != CVX_OK) return frc;
    }
    CVX_REQUIRE(d->final_gamma && d->emb && d->rope_cos && d->rope_sin && d->uniforms && d->x && d->q && d->att && d->h &&
                d->logits && d->tokens && d->state, "t2s_decode: null buffer");
    for (int l = 0; l < d->depth; ++l) {
        const cvx_t2s_layer& L = d->layers[l];
        CVX_REQUIRE(L.gamma_s && L.wqkv_s && L.wo_s && L.gamma_c && L.wq_c && L.wo_c && L.kv_c && L.gamma_f && L.w1 && L.b1 &&
                    L.w2 && L.b2 && L.k_cache && L.v_cache, "t2s_decode: null pointer in layer %d", l);
    }
    return CVX_OK;
}

extern "C" int cvx_t2s_logprob_f32(const float* logits, const int64_t* tokens, int64_t rows, int32_t V, float* out, cvx_stream_t s)
{
    CVX_REQUIRE(logits && tokens && out && rows >= 0 && rows <= 0x7fffffff && V >= 1 && V <= 1024,
                "t2s_logprob: bad arguments (rows=%lld V=%d)", (long long)rows, V);
    if (rows == 0) return CVX_OK;
    hipLaunchKernelGGL(logprob_rows_kernel, dim3((unsigned)rows), dim3(1024), 0, cvx_hip_stream(s), logits, tokens, V, out);
    CVX_CHECK_LAUNCH("cvx_t2s_logprob_f32");
    return CVX_OK;
}

// guided: BeamArgs.batch counts hypotheses - slot pairs - not slots
static BeamArgs beam_args(const cvx_t2s_decoder* d, const cvx_t2s_beam* bm, bool guided = false)
{
    return BeamArgs{d->logits, d->emb, d->x, d->state, bm->scores, bm->finished, bm->owner, bm->groups, bm->parents, bm->hist_tokens,
                    bm->hist_logprobs, bm->short_lp, bm->short_tokens, d->tokens, bm->logprobs, guided ? d->batch / 2 : d->batch, bm->beam_size,
                    d->vocab, d->dim_emb, d->streams, d->max_len};
}

static SampleArgs sample_args(const cvx_t2s_decoder* d, float* logprobs)
{
    return SampleArgs{d->logits, d->uniforms, d->emb, d->x, d->tokens, d->state, d->queue, d->dialogues, d->start, d->batch, d->uniform_steps,
                      d->vocab, d->dim_emb, d->streams, d->max_len, d->top_k, d->vocab - 1, 1.0f / fmaxf(d->temperature, 1e-10f),
                      d->cfg_scale, d->top_p, logprobs};
}

// which selection follows the logits of a step; the entry points fill it through the checks below
struct T2sSelect {
    enum Kind {
        SAMPLE,              // cvx_t2s_decode_steps, cvx_t2s_decode_steps_scored: sample_kernel
        PER,                 // cvx_t2s_decode_steps_per_dialogue: sample_per_kernel, its settings from the per-dialogue table
        MIXED,               // cvx_t2s_decode_steps_mixed: sample_mixed_kernel takes a slot's role from its record, then the scheduler - one
                             // launch more per step; n_steps == 0 runs the scheduler alone, once
        BEAM,                // cvx_t2s_beam_steps: the self-attention reads through the ancestry table, and the shortlist + merge kernels stand in
                             // for the sampling kernel - one launch more per step; every other launch is the same
        BEAM_QUEUE           // cvx_t2s_beam_queue_steps: the merge that refills its group
    } kind;
    float* logprobs;         // SAMPLE / PER / MIXED: non-NULL picks the scoring instantiation
    PerArgs per;             // PER / MIXED
    RulesArgs rules;         // PER / MIXED: a table (cvx_t2s_decode_steps_rules) picks the kernels that apply the history rules;
                             // BEAM / BEAM_QUEUE: a table (cvx_t2s_beam_rules_steps) picks the rule-aware shortlist and merge kernels
    const cvx_t2s_beam* bm;  // BEAM / BEAM_QUEUE
    BeamQueueArgs bq;        // BEAM_QUEUE
    bool guided;             // BEAM / BEAM_QUEUE: cvx_t2s_beam_guided_steps / _queue_steps - a hypothesis is a slot pair, the shortlist reads the
                             // guidance-combined row; the same number of launches
};

// the step chain of every cvx_t2s_*_steps* entry point: they differ in what follows the logits only
static int t2s_decode_run(const cvx_t2s_decoder* d, int32_t n_steps, const T2sSelect& sel, cvx_stream_t s)
{
    hipStream_t st = cvx_hip_stream(s);
    const float scale = 0.125f;        // dim_head ** -0.5
    const int nb = d->batch;
    const bool beam = sel.kind == T2sSelect::BEAM || sel.kind == T2sSelect::BEAM_QUEUE;
    const dim3 slots((unsigned)nb), block(1024);
    // ONE row pair per wave everywhere since the kernel holds 118 VGPRs (four blocks per CU): 64 slots 462 vs 480 us per CoMix step with two
    // pairs (170 VGPRs, two blocks), 32-CU side stream at 8 slots 434 vs 439 (round 5, at two blocks per CU either way, two pairs won there:
    // 760 vs 813).
    const int64_t cache_stride = (int64_t)d->max_len * d->inner;
    for (int step = 0; step < n_steps; ++step) {
        for (int l = 0; l < d->depth; ++l) {
            const cvx_t2s_layer& L = d->layers[l];
            GemvArgs g{};
            // self-attention: q | k | v with RoPE; k, v appended to the cache at position pos
            g.W = L.wqkv_s; g.ldw = d->dim; g.x = d->x; g.x_stride = d->dim; g.gamma = L.gamma_s; g.y = d->q; g.y_stride = d->inner;
            g.N = 3 * d->inner; g.K = d->dim;
            g.inner = d->inner; g.rope_cos = d->rope_cos; g.rope_sin = d->rope_sin; g.k_cache = L.k_cache; g.v_cache = L.v_cache;
            g.cache_stride = cache_stride; g.state = d->state; g.max_len = d->max_len;
            launch_gemv<MODE_QKV>(g, 3 * d->inner / 2, nb, st);
            AttnArgs at{d->q, L.k_cache, L.v_cache, d->inner, cache_stride, d->att, d->state, -1, 0, scale, d->max_len};
            if (beam) hipLaunchKernelGGL(attn_owner_kernel, dim3((unsigned)d->heads, (unsigned)nb), dim3(256), 0, st, at, (const int*)sel.bm->owner);
            else hipLaunchKernelGGL(attn_kernel, dim3((unsigned)d->heads, (unsigned)nb), dim3(256), 0, st, at);
            g = GemvArgs{};
            g.W = L.wo_s; g.ldw = d->inner; g.x = d->att; g.x_stride = d->inner; g.y = d->x; g.y_stride = d->dim; g.N = d->dim; g.K = d->inner;
            launch_gemv<MODE_RES>(g, (d->dim + 1) / 2, nb, st);
            // cross-attention over [null kv | encoder context]
            g = GemvArgs{};
            g.W = L.wq_c; g.ldw = d->dim; g.x = d->x; g.x_stride = d->dim; g.gamma = L.gamma_c; g.y = d->q; g.y_stride = d->inner;
            g.N = d->inner; g.K = d->dim;
            launch_gemv<MODE_PLAIN>(g, d->inner / 2, nb, st);
            AttnArgs ac{d->q, L.kv_c, L.kv_c + d->inner, 2 * (int64_t)d->inner, (int64_t)d->ctx_rows * 2 * d->inner, d->att, d->state,
                        d->n_ctx > 0 ? d->n_ctx : -2, 1, scale, d->max_len};
            hipLaunchKernelGGL(attn_kernel, dim3((unsigned)d->heads, (unsigned)nb), dim3(256), 0, st, ac);
            g = GemvArgs{};
            g.W = L.wo_c; g.ldw = d->inner; g.x = d->att; g.x_stride = d->inner; g.y = d->x; g.y_stride = d->dim; g.N = d->dim; g.K = d->inner;
            launch_gemv<MODE_RES>(g, (d->dim + 1) / 2, nb, st);
            // GEGLU feed-forward
            g = GemvArgs{};
            g.W = L.w1; g.ldw = d->dim; g.x = d->x; g.x_stride = d->dim; g.gamma = L.gamma_f; g.bias = L.b1; g.y = d->h;
            g.y_stride = d->ff_inner_pad; g.N = 2 * d->ff_inner; g.K = d->dim; g.y_pad = d->ff_inner_pad;
            launch_gemv<MODE_GEGLU>(g, d->ff_inner_pad, nb, st);
            g = GemvArgs{};
            g.W = L.w2; g.ldw = d->ff_inner_pad; g.x = d->h; g.x_stride = d->ff_inner_pad; g.bias = L.b2; g.y = d->x; g.y_stride = d->dim;
            g.N = d->dim; g.K = d->ff_inner_pad;
            launch_gemv<MODE_RES>(g, (d->dim + 1) / 2, nb, st);
        }
        GemvArgs g{};
        g.W = d->emb; g.ldw = d->dim_emb; g.x = d->x; g.x_stride = d->dim; g.gamma = d->final_gamma; g.y = d->logits;
        g.y_stride = d->streams * d->vocab; g.N = d->vocab; g.K = d->dim_emb; g.streams = d->streams;
        launch_gemv<MODE_LOGITS>(g, d->streams * ((d->vocab + 1) / 2), nb, st);
        if (beam && sel.guided) {
            const BeamArgs ba = beam_args(d, sel.bm, true);
            const dim3 groups((unsigned)(ba.batch / sel.bm->beam_size));
            if (sel.rules.table) {                      // cvx_t2s_beam_rules_steps: the same two launches
                if (sel.kind == T2sSelect::BEAM_QUEUE) {
                    hipLaunchKernelGGL(beam_shortlist_guided_rules_kernel<true>, dim3((unsigned)ba.batch), block, 0, st, ba, sel.bq, sel.rules, d->cfg_scale);
                    hipLaunchKernelGGL(beam_merge_guided_queue_rules_kernel, groups, block, 0, st, ba, sel.bq);
                } else {
                    hipLaunchKernelGGL(beam_shortlist_guided_rules_kernel<false>, dim3((unsigned)ba.batch), block, 0, st, ba, sel.bq, sel.rules, d->cfg_scale);
                    hipLaunchKernelGGL(beam_merge_guided_rules_kernel, groups, block, 0, st, ba);
                }
                continue;
            }
            hipLaunchKernelGGL(beam_shortlist_guided_kernel, dim3((unsigned)ba.batch), block, 0, st, ba, d->cfg_scale);
            if (sel.kind == T2sSelect::BEAM_QUEUE) hipLaunchKernelGGL(beam_merge_guided_queue_kernel, groups, block, 0, st, ba, sel.bq);
            else hipLaunchKernelGGL(beam_merge_guided_kernel, groups, block, 0, st, ba);
            continue;
        }
        if (beam) {
            const BeamArgs ba = beam_args(d, sel.bm);
            const dim3 groups((unsigned)(nb / sel.bm->beam_size));
            if (sel.rules.table) {
                if (sel.kind == T2sSelect::BEAM_QUEUE) {
                    hipLaunchKernelGGL(beam_shortlist_rules_kernel<true>, dim3((unsigned)(nb * d->streams)), block, 0, st, ba, sel.bq, sel.rules);
                    hipLaunchKernelGGL(beam_merge_queue_rules_kernel, groups, block, 0, st, ba, sel.bq);
                } else {
                    hipLaunchKernelGGL(beam_shortlist_rules_kernel<false>, dim3((unsigned)(nb * d->streams)), block, 0, st, ba, sel.bq, sel.rules);
                    hipLaunchKernelGGL(beam_merge_rules_kernel, groups, block, 0, st, ba);
                }
                continue;
            }
            hipLaunchKernelGGL(beam_shortlist_kernel, dim3((unsigned)(nb * d->streams)), block, 0, st, ba);
            if (sel.kind == T2sSelect::BEAM_QUEUE) hipLaunchKernelGGL(beam_merge_queue_kernel, groups, block, 0, st, ba, sel.bq);
            else hipLaunchKernelGGL(beam_merge_kernel, groups, block, 0, st, ba);
            continue;
        }
        const SampleArgs sa = sample_args(d, sel.logprobs);
        const bool top_p = d->filter_mode == CVX_T2S_FILTER_TOP_P;
        if (sel.rules.table) {
            if (sel.kind == T2sSelect::MIXED) {
                if (sel.logprobs) hipLaunchKernelGGL(sample_mixed_rules_kernel<true>, slots, block, 0, st, sa, sel.per, sel.rules);
                else hipLaunchKernelGGL(sample_mixed_rules_kernel<false>, slots, block, 0, st, sa, sel.per, sel.rules);
                hipLaunchKernelGGL(mixed_schedule_kernel, dim3(1), block, 0, st, sa);
            } else if (sel.logprobs) hipLaunchKernelGGL(sample_rules_kernel<true>, slots, block, 0, st, sa, sel.per, sel.rules);
            else hipLaunchKernelGGL(sample_rules_kernel<false>, slots, block, 0, st, sa, sel.per, sel.rules);
        } else if (sel.kind == T2sSelect::MIXED) {
            if (sel.logprobs) hipLaunchKernelGGL(sample_mixed_kernel<true>, slots, block, 0, st, sa, sel.per);
            else hipLaunchKernelGGL(sample_mixed_kernel<false>, slots, block, 0, st, sa, sel.per);
            hipLaunchKernelGGL(mixed_schedule_kernel, dim3(1), block, 0, st, sa);
        } else if (sel.kind == T2sSelect::PER) {
            if (sel.logprobs) hipLaunchKernelGGL(sample_per_kernel<true>, slots, block, 0, st, sa, sel.per);
            else hipLaunchKernelGGL(sample_per_kernel<false>, slots, block, 0, st, sa, sel.per);
        } else if (sel.logprobs) {
            if (top_p) hipLaunchKernelGGL((sample_kernel<FILT_TOP_P, true>), slots, block, 0, st, sa);
            else hipLaunchKernelGGL((sample_kernel<FILT_TOP_K, true>), slots, block, 0, st, sa);
        } else if (top_p) hipLaunchKernelGGL(sample_kernel<FILT_TOP_P>, slots, block, 0, st, sa);
        else hipLaunchKernelGGL(sample_kernel<FILT_TOP_K>, slots, block, 0, st, sa);
    }
    if (sel.kind == T2sSelect::MIXED && n_steps == 0) hipLaunchKernelGGL(mixed_schedule_kernel, dim3(1), block, 0, st, sample_args(d, sel.logprobs));
    CVX_CHECK_LAUNCH("cvx_t2s_decode_steps");
    return CVX_OK;
}

// ---- the argument checks the entry points share.  `who`: the entry point's name in the message.  Each runs behind t2s_validate (it reads the
// descriptor), refuses with CVX_EINVAL before anything is launched, and fills its part of the selection.
#define T2S_TRY(call)                        \
    do {                                     \
        const int rc_ = (call);              \
        if (rc_ != CVX_OK) return rc_;       \
    } while (0)

template <class T>
static int t2s_struct_size(const char* who, const char* type, const T* p)
{
    CVX_REQUIRE(p && p->struct_size == sizeof(T), "%s: %s.struct_size = %u, this library knows %u", who, type, p ? p->struct_size : 0u,
                (unsigned)sizeof(T));
    return CVX_OK;
}

// cvx_t2s_scoring; optional: none (NULL) leaves the log-prob epilogue off
static int t2s_scoring_block(const char* who, const cvx_t2s_decoder* d, const cvx_t2s_scoring* sc, bool optional, T2sSelect& sel)
{
    if (optional && !sc) return CVX_OK;
    T2S_TRY(t2s_struct_size(who, "cvx_t2s_scoring", sc));
    CVX_REQUIRE(sc->logprobs, "%s: null logprobs", who);
    CVX_REQUIRE(sc->logprob_len == d->max_len, "%s: logprob_len = %d, the rows of logprobs are laid out like those of tokens (max_len = %d floats)",
                who, sc->logprob_len, d->max_len);
    sel.logprobs = sc->logprobs;
    return CVX_OK;
}

// cvx_t2s_per_dialogue: every record a slot can name has a row - the n_dialogues behind a queue; without one, slot b decodes dialogue b
static int t2s_per_dialogue_block(const char* who, const cvx_t2s_decoder* d, const cvx_t2s_per_dialogue* per, T2sSelect& sel)
{
    T2S_TRY(t2s_struct_size(who, "cvx_t2s_per_dialogue", per));
    CVX_REQUIRE(per->table && per->n_records >= 1, "%s: null table or n_records = %d < 1", who, per->n_records);
    CVX_REQUIRE(per->n_records >= d->n_dialogues && (d->queue || per->n_records >= d->batch),
                "%s: n_records = %d rows for %d dialogue records / %d slots", who, per->n_records, d->n_dialogues, d->batch);
    sel.per = PerArgs{static_cast<const int*>(per->table), per->n_records};
    return CVX_OK;
}

// cvx_t2s_beam.  guided: the entry points whose hypotheses are slot pairs (t2s_validate has held cfg_scale > 1 to one stream, an even
// batch and n_ctx == 0)
static int t2s_beam_block(const char* who, const cvx_t2s_decoder* d, const cvx_t2s_beam* bm, T2sSelect& sel, bool guided = false)
{
    T2S_TRY(t2s_struct_size(who, "cvx_t2s_beam", bm));
    CVX_REQUIRE(!d->queue, "%s: the dialogue queue of the sampled decode cannot feed beam groups (dec->queue must be NULL)", who);
    if (guided)
        CVX_REQUIRE(d->cfg_scale > 1.f && d->streams == 1 && d->n_ctx == 0,
                    "%s: cfg_scale = %g must be > 1 (cvx_t2s_beam_steps is the unguided entry) on a one-output model with per-slot context "
                    "rows (streams = %d, n_ctx = %d)", who, (double)d->cfg_scale, d->streams, d->n_ctx);
    else
        CVX_REQUIRE(!(d->cfg_scale > 1.f), "%s: guidance (cfg_scale > 1) runs through %s", who,
                    sel.kind == T2sSelect::BEAM_QUEUE ? "cvx_t2s_beam_guided_queue_steps" : "cvx_t2s_beam_guided_steps");
    const int per = guided ? 2 : 1;                    // slots per hypothesis
    CVX_REQUIRE(bm->beam_size >= 1 && bm->beam_size <= BEAM_MAX && d->batch % (per * bm->beam_size) == 0,
                "%s: beam_size = %d outside [1, %d], or %d slots per utterance do not divide batch = %d", who, bm->beam_size, BEAM_MAX,
                per * bm->beam_size, d->batch);
    CVX_REQUIRE(bm->hist_len == d->max_len, "%s: hist_len = %d, the history arrays and logprobs hold max_len = %d steps", who, bm->hist_len,
                d->max_len);
    CVX_REQUIRE(bm->scores && bm->finished && bm->owner && bm->groups && bm->parents && bm->hist_tokens && bm->hist_logprobs && bm->short_lp &&
                bm->short_tokens && bm->logprobs, "%s: null pointer in cvx_t2s_beam", who);
    sel.bm = bm;
    sel.guided = guided;
    return CVX_OK;
}

extern "C" int cvx_t2s_decode_steps(const cvx_t2s_decoder* d, int32_t n_steps, cvx_stream_t s)
{
    T2S_TRY(t2s_validate(d, n_steps));
    return t2s_decode_run(d, n_steps, T2sSelect{T2sSelect::SAMPLE}, s);
}

extern "C" int cvx_t2s_decode_steps_scored(const cvx_t2s_decoder* d, const cvx_t2s_scoring* sc, int32_t n_steps, cvx_stream_t s)
{
    T2sSelect sel{T2sSelect::SAMPLE};
    T2S_TRY(t2s_validate(d, n_steps));
    T2S_TRY(t2s_scoring_block("t2s_decode_scored", d, sc, false, sel));
    return t2s_decode_run(d, n_steps, sel, s);
}

extern "C" int cvx_t2s_decode_steps_per_dialogue(const cvx_t2s_decoder* d, const cvx_t2s_scoring* sc, const cvx_t2s_per_dialogue* per,
                                                 int32_t n_steps, cvx_stream_t s)
{
    const char* const who = "t2s_decode_per_dialogue";
    T2sSelect sel{T2sSelect::PER};
    T2S_TRY(t2s_validate(d, n_steps, true));
    T2S_TRY(t2s_per_dialogue_block(who, d, per, sel));
    T2S_TRY(t2s_scoring_block(who, d, sc, true, sel));
    return t2s_decode_run(d, n_steps, sel, s);
}

// cvx_t2s_mixed, with the settings table and the optional scoring block of the mixed chain
static int t2s_mixed_block(const char* who, const cvx_t2s_decoder* d, const cvx_t2s_scoring* sc, const cvx_t2s_per_dialogue* per,
                           const cvx_t2s_mixed* mx, T2sSelect& sel)
{
    T2S_TRY(t2s_struct_size(who, "cvx_t2s_mixed", mx));
    CVX_REQUIRE(d->queue, "%s: the scheduler hands out records from the dialogue queue (queue must not be NULL)", who);
    CVX_REQUIRE(!(d->cfg_scale > 1.f), "%s: cfg_scale = %g > 1 asks for the launch-wide pair layout; here the layout is per "
                "record (flag bit 2) and the scale comes from the table", who, (double)d->cfg_scale);
    T2S_TRY(t2s_per_dialogue_block(who, d, per, sel));
    T2S_TRY(t2s_scoring_block(who, d, sc, true, sel));
    CVX_REQUIRE(mx->n_guided >= 0 && 2 * (int64_t)mx->n_guided <= d->n_dialogues,
                "%s: n_guided = %d guided utterances take two records each of the %d", who, mx->n_guided, d->n_dialogues);
    CVX_REQUIRE(mx->n_guided == 0 || (d->streams == 1 && d->batch >= 2),
                "%s: guided records need a one-output model and two slots (streams = %d, batch = %d)", who, d->streams, d->batch);
    return CVX_OK;
}

extern "C" int cvx_t2s_decode_steps_mixed(const cvx_t2s_decoder* d, const cvx_t2s_scoring* sc, const cvx_t2s_per_dialogue* per,
                                          const cvx_t2s_mixed* mx, int32_t n_steps, cvx_stream_t s)
{
    const char* const who = "t2s_decode_mixed";
    T2sSelect sel{T2sSelect::MIXED};
    T2S_TRY(t2s_validate(d, n_steps, true));
    T2S_TRY(t2s_mixed_block(who, d, sc, per, mx, sel));
    return t2s_decode_run(d, n_steps, sel, s);
}

// the per-dialogue chain (mx == NULL) or the mixed chain under the history rules: one rules row per row of the settings table
extern "C" int cvx_t2s_decode_steps_rules(const cvx_t2s_decoder* d, const cvx_t2s_scoring* sc, const cvx_t2s_per_dialogue* per,
                                          const cvx_t2s_mixed* mx, const cvx_t2s_rules* ru, int32_t n_steps, cvx_stream_t s)
{
    const char* const who = "t2s_decode_rules";
    T2sSelect sel{mx ? T2sSelect::MIXED : T2sSelect::PER};
    T2S_TRY(t2s_validate(d, n_steps, true));
    if (mx) T2S_TRY(t2s_mixed_block(who, d, sc, per, mx, sel));
    else {
        T2S_TRY(t2s_per_dialogue_block(who, d, per, sel));
        T2S_TRY(t2s_scoring_block(who, d, sc, true, sel));
    }
    T2S_TRY(t2s_struct_size(who, "cvx_t2s_rules", ru));
    CVX_REQUIRE(ru->table && ru->n_records >= 1, "%s: null rules table or n_records = %d < 1", who, ru->n_records);
    CVX_REQUIRE(ru->n_records >= d->n_dialogues && (d->queue || ru->n_records >= d->batch),
                "%s: rules n_records = %d rows for %d dialogue records / %d slots", who, ru->n_records, d->n_dialogues, d->batch);
    sel.rules = RulesArgs{static_cast<const int*>(ru->table), ru->n_records};
    return t2s_decode_run(d, n_steps, sel, s);
}

extern "C" int cvx_t2s_rules_f32(const float* logits, const int64_t* history, const int32_t* hist_len, const void* table, int64_t rows,
                                 int32_t V, int32_t hist_ld, int32_t eos_id, float* out, cvx_stream_t s)
{
    CVX_REQUIRE(logits && hist_len && table && out && rows >= 0 && rows <= 0x7fffffff && V >= 1 && V <= 1024 && hist_ld >= 0 &&
                (history || hist_ld == 0), "t2s_rules: bad arguments (rows=%lld V=%d hist_ld=%d)", (long long)rows, V, hist_ld);
    if (rows == 0) return CVX_OK;
    const RulesRowsArgs a{logits, history, hist_len, static_cast<const int*>(table), out, V, hist_ld, eos_id};
    hipLaunchKernelGGL(rules_rows_kernel, dim3((unsigned)rows), dim3(1024), 0, cvx_hip_stream(s), a);
    CVX_CHECK_LAUNCH("cvx_t2s_rules_f32");
    return CVX_OK;
}

// cvx_t2s_beam_steps and cvx_t2s_beam_guided_steps: the checks, the steps, the back-track (one thread per hypothesis)
// cvx_t2s_rules of cvx_t2s_beam_rules_steps (rules: whether the entry point takes one): a row per utterance - `rows` of them
static int t2s_beam_rules_block(const char* who, const cvx_t2s_rules* ru, bool rules, int rows, T2sSelect& sel)
{
    if (!rules) return CVX_OK;
    T2S_TRY(t2s_struct_size(who, "cvx_t2s_rules", ru));
    CVX_REQUIRE(ru->table && ru->n_records >= 1 && ru->n_records >= rows, "%s: null rules table, or n_records = %d rows for %d utterances", who,
                ru->n_records, rows);
    sel.rules = RulesArgs{static_cast<const int*>(ru->table), ru->n_records};
    return CVX_OK;
}

// (rules: the entry point is cvx_t2s_beam_rules_steps, which is guided by the descriptor's scale - read once t2s_validate has passed it)
static int t2s_beam_steps(const char* who, const cvx_t2s_decoder* d, const cvx_t2s_beam* bm, int32_t n_steps, bool guided, cvx_stream_t s,
                          const cvx_t2s_rules* ru = nullptr, bool rules = false)
{
    T2sSelect sel{T2sSelect::BEAM};
    T2S_TRY(t2s_validate(d, n_steps));
    if (rules) guided = d->cfg_scale > 1.f;
    T2S_TRY(t2s_beam_block(who, d, bm, sel, guided));
    T2S_TRY(t2s_beam_rules_block(who, ru, rules, d->batch / ((guided ? 2 : 1) * bm->beam_size), sel));
    if (n_steps > 0) T2S_TRY(t2s_decode_run(d, n_steps, sel, s));
    if (bm->backtrack) {
        const BeamArgs ba = beam_args(d, bm, guided);
        hipLaunchKernelGGL(beam_backtrack_kernel, dim3((unsigned)((ba.batch + 63) / 64)), dim3(64), 0, cvx_hip_stream(s), ba);
        CVX_CHECK_LAUNCH(who);
    }
    return CVX_OK;
}

extern "C" int cvx_t2s_beam_steps(const cvx_t2s_decoder* d, const cvx_t2s_beam* bm, int32_t n_steps, cvx_stream_t s)
{
    return t2s_beam_steps("t2s_beam_steps", d, bm, n_steps, false, s);
}

extern "C" int cvx_t2s_beam_guided_steps(const cvx_t2s_decoder* d, const cvx_t2s_beam* bm, int32_t n_steps, cvx_stream_t s)
{
    return t2s_beam_steps("t2s_beam_guided_steps", d, bm, n_steps, true, s);
}

// cvx_t2s_beam_queue_steps and cvx_t2s_beam_guided_queue_steps
static int t2s_beam_queue_steps(const char* who, const cvx_t2s_decoder* d, const cvx_t2s_beam* bm, const cvx_t2s_beam_queue* bq, int32_t n_steps,
                                bool guided, cvx_stream_t s, const cvx_t2s_rules* ru = nullptr, bool rules = false)
{
    T2sSelect sel{T2sSelect::BEAM_QUEUE};
    T2S_TRY(t2s_validate(d, n_steps));
    if (rules) guided = d->cfg_scale > 1.f;                    // (as in t2s_beam_steps)
    T2S_TRY(t2s_beam_block(who, d, bm, sel, guided));
    T2S_TRY(t2s_struct_size(who, "cvx_t2s_beam_queue", bq));
    CVX_REQUIRE(bq->n_utterances >= 1, "%s: n_utterances = %d", who, bq->n_utterances);
    CVX_REQUIRE(bq->queue && bq->utterances && bq->start && bq->parents && bq->hist_tokens && bq->hist_logprobs && bq->final_scores &&
                bq->final_steps && bq->final_finished && bq->tokens && bq->logprobs, "%s: null pointer in cvx_t2s_beam_queue", who);
    T2S_TRY(t2s_beam_rules_block(who, ru, rules, bq->n_utterances, sel));
    sel.bq = BeamQueueArgs{bq->queue, bq->utterances, bq->start, bq->parents, bq->hist_tokens, bq->hist_logprobs, bq->final_scores,
                           bq->final_steps, bq->final_finished, bq->tokens, bq->logprobs, bq->n_utterances, d->ctx_rows};
    if (n_steps > 0) T2S_TRY(t2s_decode_run(d, n_steps, sel, s));
    if (bm->backtrack) {
        hipLaunchKernelGGL(beam_backtrack_queue_kernel, dim3((unsigned)(((int64_t)bq->n_utterances * bm->beam_size + 63) / 64)), dim3(64), 0,
                           cvx_hip_stream(s), beam_args(d, bm, guided), sel.bq);
        CVX_CHECK_LAUNCH(who);
    }
    return CVX_OK;
}

extern "C" int cvx_t2s_beam_queue_steps(const cvx_t2s_decoder* d, const cvx_t2s_beam* bm, const cvx_t2s_beam_queue* bq, int32_t n_steps,
                                        cvx_stream_t s)
{
    return t2s_beam_queue_steps("t2s_beam_queue_steps", d, bm, bq, n_steps, false, s);
}

extern "C" int cvx_t2s_beam_guided_queue_steps(const cvx_t2s_decoder* d, const cvx_t2s_beam* bm, const cvx_t2s_beam_queue* bq, int32_t n_steps,
                                               cvx_stream_t s)
{
    return t2s_beam_queue_steps("t2s_beam_guided_queue_steps", d, bm, bq, n_steps, true, s);
}

// the four beam chains under the history rules: lock-step (bq == NULL) or refilled, guided when dec->cfg_scale > 1
extern "C" int cvx_t2s_beam_rules_steps(const cvx_t2s_decoder* d, const cvx_t2s_beam* bm, const cvx_t2s_beam_queue* bq, const cvx_t2s_rules* ru,
                                        int32_t n_steps, cvx_stream_t s)
{
    const char* const who = "t2s_beam_rules_steps";
    if (bq) return t2s_beam_queue_steps(who, d, bm, bq, n_steps, false, s, ru, true);
    return t2s_beam_steps(who, d, bm, n_steps, false, s, ru, true);
}

extern "C" int cvx_t2s_beam_select_rules_f32(const float* logits, const float* scores_in, const uint8_t* finished_in, const int32_t* history,
                                             const int32_t* hist_len, const void* table, int32_t groups, int32_t beam_size, int32_t streams,
                                             int32_t V, int32_t hist_ld, int32_t* parents, int64_t* tokens, float* token_lp, float* scores_out,
                                             uint8_t* finished_out, cvx_stream_t s)
{
    CVX_REQUIRE(logits && scores_in && finished_in && hist_len && table && parents && tokens && token_lp && scores_out && finished_out &&
                (history || hist_ld == 0), "t2s_beam_select_rules: null pointer");
    CVX_REQUIRE(groups >= 0 && beam_size >= 1 && beam_size <= BEAM_MAX && (streams == 1 || streams == 2) && V >= 1 && V <= 1024 &&
                hist_ld >= 0 && hist_ld <= T2S_MAX_KEYS,
                "t2s_beam_select_rules: bad arguments (groups=%d beam_size=%d streams=%d V=%d hist_ld=%d)", groups, beam_size, streams, V, hist_ld);
    if (groups == 0) return CVX_OK;
    const BeamSelectArgs a{logits, scores_in, finished_in, beam_size, streams, V, parents, tokens, token_lp, scores_out, finished_out};
    const BeamSelectRulesArgs ra{history, hist_len, static_cast<const int*>(table), hist_ld};
    hipLaunchKernelGGL(beam_select_rules_kernel, dim3((unsigned)groups), dim3(1024), 0, cvx_hip_stream(s), a, ra);
    CVX_CHECK_LAUNCH("cvx_t2s_beam_select_rules_f32");
    return CVX_OK;
}

extern "C" int cvx_t2s_beam_select_f32(const float* logits, const float* scores_in, const uint8_t* finished_in, int32_t groups,
                                       int32_t beam_size, int32_t streams, int32_t V, int32_t* parents, int64_t* tokens, float* token_lp,
                                       float* scores_out, uint8_t* finished_out, cvx_stream_t s)
{
    CVX_REQUIRE(logits && scores_in && finished_in && parents && tokens && token_lp && scores_out && finished_out,
                "t2s_beam_select: null pointer");
    CVX_REQUIRE(groups >= 0 && beam_size >= 1 && beam_size <= BEAM_MAX && (streams == 1 || streams == 2) && V >= 1 && V <= 1024,
                "t2s_beam_select: bad arguments (groups=%d beam_size=%d streams=%d V=%d)", groups, beam_size, streams, V);
    if (groups == 0) return CVX_OK;
    const BeamSelectArgs a{logits, scores_in, finished_in, beam_size, streams, V, parents, tokens, token_lp, scores_out, finished_out};
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)groups), dim3(1024), 0, cvx_hip_stream(s), a);
    CVX_CHECK_LAUNCH("cvx_t2s_beam_select_f32");
    return CVX_OK;
}
