/* covomix_hip.h - C ABI of libcovomix_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary of the build.  The reference has no native
 * code on this path - its contract is the PyTorch semantics of the modules cited
 * below (paths relative to /root/reference) - so every entry point here names the
 * reference computation it replaces.  Conventions:
 *   - plain C symbols; device pointers + explicit shapes/strides; a hipStream_t
 *     (passed as void*) on which the work is enqueued; no hidden allocation, no
 *     global mutable state besides a thread-local last-error string;
 *   - return 0 on success, CVX_EINVAL on a shape/alignment error, CVX_EHIP when
 *     the HIP runtime reported a launch error (message via cvx_last_error_string);
 *   - all floating-point data is fp32 row-major; token ids are int64.
 * Weights are borrowed (never copied or freed by the library).
 */
#ifndef COVOMIX_HIP_H
#define COVOMIX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVX_OK      0
#define CVX_EINVAL (-22)
#define CVX_EHIP   (-5)

#define CVX_ACT_NONE 0
#define CVX_ACT_GELU 1   /* exact erf GELU  (nn.GELU default, acoustic.py:159,244) */
#define CVX_ACT_SILU 2   /* SiLU            (time MLP, acoustic.py:364)            */
#define CVX_ACT_TANH 3

/* LAUNCH CONTEXT (version 107): what every entry point takes where it used to take a bare hipStream_t.  A plain host struct the
 * CALLER owns and may keep for the life of the stream; the library only reads it during the call and keeps NOTHING about a stream
 * between calls (no table, no lock: re-entrant per context; SURVEY.md section 8(b) "no global mutable state").  NULL = the null
 * stream, no flag, the whole device. */
typedef struct cvx_ctx {
    void*     stream;     /* hipStream_t the call launches on */
    uint32_t* sat_flag;   /* the sticky saturation flag of this stream: one 4-byte aligned uint32 of DEVICE memory the caller zeroed and
                           * keeps alive (below), or NULL */
    int32_t   n_cus;      /* compute units the stream owns (a CU-masked stream, cvx_stream_create_cu_mask); 0 = the device's: what the
                           * persistent grids and the large / medium GEMM choice are sized from */
    int32_t   flags;      /* CVX_CTX_* */
} cvx_ctx;
#define CVX_CTX_NO_SATURATION_FLAG 1   /* run the calls that write split (fp16 hi, lo) pairs WITHOUT the saturation bookkeeping: without
                                        * this bit such a call refuses a context whose sat_flag is NULL (CVX_EINVAL) - a C caller cannot
                                        * lose the safety net by forgetting it */
typedef const cvx_ctx* cvx_stream_t;

/* ABI version of the library: CVX_ABI_VERSION of the header it was built from.  The argument structs carry no size field, so a
 * caller built against another header version must not call in: compare once after loading (the ctypes binding does,
 * covomix_amd/_lib.py).  104: round 4 (cvx_gemm_f16x3_norm, caller-owned saturation flags, cvx_t2s_decoder.cfg_scale,
 * cvx_t2s_decode_xcd, CVX_GEMM_FLAG_MEDIUM / _NO_MEDIUM).  105: round 4, the deferred AdaptiveRMSNorm - cvx_gemm_split_io grew
 * c_gamma_dev ... a2_scale_dev at its end; cvx_rownorm_scale_f32, cvx_split_f16_colscale_il.  106: round 5 - CU-partitioned
 * streams (cvx_stream_create_cu_mask / _destroy / cvx_stream_set_cus / cvx_stream_cus); the library reads no environment
 * variable in any build; REMOVED (measured slower, numbers in
 * HISTORY.md): cvx_t2s_decode_persistent, cvx_t2s_decode_xcd, cvx_embed_conv31_f32, CVX_GEMM_FLAG_TWO_STAGE / _MFMA32 (the superseded
 * large-problem GEMM forms: shapes the eight-phase kernel cannot take run on the 128 x 128 kernel).  107: round 6 - text2semantic
 * decode of up to 64 slots at independent positions with an on-device dialogue queue (continuous batching): cvx_t2s_decoder grew
 * uniform_steps / queue / dialogues / start, slot records are int32[8], uniforms and tokens are indexed by dialogue; every entry point
 * takes a LAUNCH CONTEXT (cvx_ctx: stream + caller-owned saturation flag + CU count) instead of a bare stream - REMOVED: the library's
 * (device, stream) table and cvx_saturation_flag_bind / cvx_stream_set_cus / cvx_stream_cus.  108: cvx_t2s_decoder loses its
 * last two fields, the tuning hints group_loop and pairs_per_wave (the decode takes one row pair per wavefront and one group of
 * slots per thread block).  109: cvx_attention_f16x3_form (which kernel form a split-precision attention launch takes; host
 * arithmetic only, so that tests can place a problem on every form).  110: CVX_ATT_FORM_D (256-query blocks, two query sets per
 * wave, for launches of 512 such blocks and more); CVX_ATT_FORM_SINGLE_TERM is 4 (was 3).  111: text2semantic sampling controls -
 * cvx_t2s_decoder grew filter_mode / top_p / n_dialogues at its end (top-p beside top-k), a dialogue queue may run under guidance
 * (record pairs), cvx_t2s_sample_f32 (the filter + sampling of one decode step on caller-supplied logits).  112:
 * cvx_hifigan_conv1d_f16x3_form (the tile height a split-precision convolution launch takes; host arithmetic only, so that tests can
 * place a problem on every tile form).  113: cvx_gemm_f32_form (which of its four kernels an fp32 GEMM launch takes; host arithmetic
 * only, so that tests can place a problem on every kernel).  Still 113 (symbols added, no struct or entry point changed): cvx_t2s_beam_steps
 * with its own size-carrying struct, cvx_t2s_beam_select_f32 - beam search on the decode slots; cvx_t2s_beam_queue_steps with
 * cvx_t2s_beam_queue - beam search through continuously refilled slot groups.  Still 113 (additive, one formerly ignored
 * flag bit; no struct or entry point changes): the V^T stores of a to_qkv launch of the eight-phase kernels go line-major, 16 bytes
 * per lane (same values, same addresses); CVX_GEMM_FLAG_VT_PIECES keeps the earlier store code selectable.  Still 113 (a symbol and a
 * struct added): cvx_t2s_decode_steps_mixed with cvx_t2s_mixed - guided and unguided dialogues in one slot pool; slot record [7], so
 * far reserved, carries a slot's role there.  Still 113 (two symbols added, no struct changed): cvx_t2s_beam_guided_steps and
 * cvx_t2s_beam_guided_queue_steps - beam search under classifier-free guidance, on the structs of the unguided entry points.  Still 113
 * (two symbols and a struct added): cvx_t2s_decode_steps_rules with cvx_t2s_rules, cvx_t2s_rules_f32 - repetition penalty, no-repeat
 * n-gram and minimum length per dialogue; cvx_t2s_per_dialogue and its rows are untouched.  Still 113 (two symbols added, no struct
 * changed): cvx_t2s_beam_rules_steps and cvx_t2s_beam_select_rules_f32 - no-repeat n-gram and minimum length under beam search.  Still 113
 * (six symbols added, no struct changed): cvx_mel_items_words / _fill, cvx_mel_pack_f32, cvx_mel_log_gather_f32,
 * cvx_mel_workspace_bytes_many and cvx_mel_spectrogram_many_f32 - the prompt mel of many wav prompts in one call. */
#define CVX_ABI_VERSION 113
int         cvx_version(void);
const char* cvx_last_error_string(void);

/* ------------------------------------------------------------------------
 * Sticky saturation flag: CALLER-OWNED, one uint32 of device memory per stream, carried by the launch context (cvx_ctx.sat_flag;
 * versions 104-106 kept a (device, stream) -> flag table inside the library, until 102 the library allocated one per device).
 * The split-precision path stores activations as (fp16 hi, fp16 lo) pairs times a power-of-two pre-scale chosen so that
 * the tensor's expected RMS sits at 2^4 (transformer: a weights-only gain model) or its measured max at 2^10 (vocoder):
 * 2^12 resp. 2^6 of headroom before `hi` saturates at 65504.  A checkpoint with one outlier row / channel can leave that
 * window; the pair is then CLAMPED and no longer represents the fp32 value.  Every kernel that writes split pairs (GEMM
 * epilogues incl. the transposed V^T store, AdaRMSNorm, attention, cvx_split_f16*, the HiFi-GAN convolutions and layout
 * converter) ORs bit 0 into the flag OF THE CONTEXT IT IS LAUNCHED WITH when a value it stored exceeded 65504 in magnitude
 * (the attention kernel also when a softmax normaliser is not a positive finite number).  The flag is never cleared by a kernel:
 * reset it, run any number of calls, query once.  The host path (CoVoMixModel.synthesis_sample, Generator.__call__) does exactly
 * that and re-runs the call on the exact-fp32 kernels when the flag is set - a saturated result is never returned silently.
 * Several contexts may share one flag (the side stream of a two-stream schedule, a graph-capture stream).  A call that writes
 * pairs with a context that has no flag returns CVX_EINVAL unless the context says CVX_CTX_NO_SATURATION_FLAG.
 *   cvx_saturation_flag_reset: enqueue a clear of the context's flag on its stream (no host synchronisation); CVX_EINVAL without one.
 *   cvx_saturation_flag_query: copy the flag to *host_out behind everything enqueued on the stream (SYNCHRONISES it), then
 *                              optionally enqueue a clear. */
int cvx_saturation_flag_reset(cvx_stream_t ctx);
int cvx_saturation_flag_query(uint32_t* host_out, int32_t reset, cvx_stream_t ctx);

/* ------------------------------------------------------------------------
 * CU-partitioned streams (round 5): the text2semantic decode of the NEXT batch of dialogues (a latency chain of 34 dependent
 * launches per token that needs a handful of CUs; reference loop dialogue_generation.py:272-329, decode
 * covomix/covomix_model/text2semantic.py:749-848) can run UNDER the acoustic solve of the current one.  The large-problem GEMM is a
 * persistent kernel that owns every CU it gets for a whole launch, so a plain side stream would only be served at launch
 * boundaries: the two stages run on streams restricted to DISJOINT CU sets instead.
 *   cvx_stream_create_cu_mask: hipExtStreamCreateWithCUMask -> *out_stream (a hipStream_t the caller owns; put it into a cvx_ctx
 *                              together with n_cus = the number of mask bits).  Bit k of the mask names CU (k / 8) of XCD (k % 8);
 *                              inside an XCD consecutive indices go round the four shader engines (measured on MI355X,
 *                              tools/archive/cu_mask_probe.hip).  One-block-per-CU kernels are only co-resident when every shader engine keeps
 *                              the same number of CUs, i.e. when the CUs per XCD are a multiple of 4 (tools/archive/cu_mask_probe2.hip: 30 CUs
 *                              per XCD -> 12 of 240 blocks wait for a second round; 28 -> none).
 *   cvx_stream_destroy:        hipStreamDestroy of such a stream. */
/* Diagnostics (bench.py): stamps_dev is 2048 x 2 uint64 of ZEROED device memory; slot = xcd * 256 + HW_ID[15:8] (the CU's id bits) receives
 * {that CU's shader-clock cycle counter, the 100 MHz real-time counter} (slots of CUs no block landed on stay zero).  Two calls around a
 * busy region, paired slot by slot (the cycle counters of different CUs are not comparable) -> the shader clock the region ran at, per CU. */
int cvx_clock_stamps(uint64_t* stamps_dev, cvx_stream_t ctx);
int cvx_stream_create_cu_mask(const uint32_t* mask, int32_t n_words, void** out_stream);
int cvx_stream_destroy(void* stream);

/* ------------------------------------------------------------------------
 * C[M,N] = epilogue( [A | A2][M,K] * W[N,K]^T )      fp32 MFMA (v_mfma_f32_32x32x2_f32)
 *
 * Replaces every nn.Linear on the path: to_embed (acoustic.py:503-505), to_qkv /
 * to_out (:225-237), FeedForward (:241-246), skip combiner on cat(x, skip)
 * (:306-310, expressed as a K-split over two inputs: columns [0,K1) come from A,
 * [K1,K) from A2), to_pred (:516), the time MLP (:361-365) and the to_gamma /
 * to_beta projections (:200).
 * epilogue order:  v = acc + bias[n];  v = act(v);
 *                  RoPE (half-split, acoustic.py:132-137) on columns [0,rope_cols):
 *                       64-wide heads, position = row % rope_T, tables cos/sin[rope_T][32];
 *                  v += residual[m,n];  C[m,n] = v.
 * Requirements: K % 4 == 0, lda/lda2/ldw % 4 == 0, 16-byte aligned A/A2/W,
 *               K1 % 32 == 0 when A2 != NULL, rope_cols % 64 == 0.
 */
typedef struct {
    const float* A;   int64_t lda;
    const float* A2;  int64_t lda2;  int32_t K1;
    const float* W;   int64_t ldw;
    float*       C;   int64_t ldc;
    const float* bias;
    const float* residual; int64_t ldr;
    int32_t M, N, K;
    int32_t act;
    const float* rope_cos; const float* rope_sin; int32_t rope_T; int32_t rope_cols;
} cvx_gemm_args;
int cvx_gemm_bias_act_f32(const cvx_gemm_args* a, cvx_stream_t s);

/* Which kernel cvx_gemm_bias_act_f32 launches for a shape: the launcher takes its decision from this very function.  No GPU work,
 * no stream, callable on a machine without a GPU.  -1 for a shape no launch can have (M < 1, N < 1, K < 4 or K % 4 != 0).
 *   T64:          64-row tiles, operands staged through registers  (K % 32 == 0; M <= 64, or fewer than 256 tiles of 128 x 128)
 *   T64_GENERIC:  64-row tiles, predicated loads                   (the same shapes with K % 32 != 0)
 *   T128_DMA:     128-row tiles, operands by LDS-DMA               (K % 32 == 0, M > 64, 256 tiles of 128 x 128 and more)
 *   T128_GENERIC: 128-row tiles, predicated loads                  (the same shapes with K % 32 != 0)
 * The four agree to fp32 rounding, not bit for bit. */
#define CVX_GEMM_F32_FORM_T64          0
#define CVX_GEMM_F32_FORM_T64_GENERIC  1
#define CVX_GEMM_F32_FORM_T128_DMA     2
#define CVX_GEMM_F32_FORM_T128_GENERIC 3
int cvx_gemm_f32_form(int32_t M, int32_t N, int32_t K);

/* Split-precision variant of the same contract (same nn.Linear call sites): every fp32 operand is an
 * (fp16 hi, fp16 lo) pair, hi = fp16(x), lo = fp16(x - hi), and  a*w ~= a_hi*w_hi + a_hi*w_lo + a_lo*w_hi
 * on v_mfma_f32_32x32x16_f16 with fp32 accumulation (~2^-22 relative operand error, inputs saturated to
 * +-65504).  W_hi / W_lo are [N, a->ldw] fp16 matrices produced once by cvx_split_f16 from the fp32 weight
 * (a->W is only validated, not read).  Extra requirements: K % 32 == 0, ldw % 8 == 0.
 * cvx_split_f16 splits w*scale (scale = a power of two that lifts small weights out of the fp16 subnormal
 * range); cvx_gemm_f16x3 multiplies the accumulators by acc_scale = 1/scale (exact) before the epilogue.
 * `io` (may be NULL) lets activations stay in split form between kernels: A_hi/A_lo (and A2_*) give the A operand
 * already split (then a->A / a->A2 are only validated and every tile arrives by LDS-DMA); C_hi/C_lo receive a split
 * copy of the output for the next GEMM, and write_f32 == 0 drops the fp32 store of C altogether.
 *
 * Interleaved pairs.  Wherever this header takes an (fp16 hi, fp16 lo) pair of a row-major activation - A_*, A2_*,
 * C_* here, y_hi/y_lo of cvx_adarmsnorm_f32, out_hi/out_lo of cvx_attention_f32 / cvx_attention_f16x3, hi/lo of
 * cvx_split_f16 - passing lo == hi + 32 (halves) selects ONE buffer of row length 2*cols in which every block of 32
 * values is stored as [hi 32 | lo 32]: flat offset o of the two-tensor form lives at ((o >> 5) << 6) | (o & 31) for
 * hi and 32 halves later for lo; the leading dimension (lda_h, ldc_h) is then the row length of that buffer in
 * halves (>= 2*cols).  Values are bit-identical to the two-tensor form; the layout makes one K-step of a row one
 * 128-byte cache line.  cvx_gemm_f16x3 reads interleaved A/A2 only in the large-problem kernel (M >= 2048,
 * N >= 512) and only together with w_interleaved; A and A2 must then both be interleaved.  lo == NULL always means
 * "hi only" (single-term fp16). */
typedef struct {
    const uint16_t* A_hi;  const uint16_t* A_lo;  int64_t lda_h;
    const uint16_t* A2_hi; const uint16_t* A2_lo; int64_t lda2_h;
    uint16_t* C_hi; uint16_t* C_lo; int64_t ldc_h;
    int32_t write_f32;
    /* QKV mode (optional; needs the RoPE arguments, N = 3*H*64, write_f32 = 0; T % 4 != 0 is accepted but stores the v columns 2 bytes at a time): the v columns are not
     * written to C_hi/C_lo but TRANSPOSED per (sequence, head) to Vt_*[((b*H + h)*64 + d) * vt_ld + slot(t)] (slot swaps bits 2 and 3
     * of t: four-frame groups in the order 0, 2, 1, 3 inside every 16 frames), the layout
     * cvx_attention_f16x3 reads its V^T tiles from. */
    uint16_t* Vt_hi; uint16_t* Vt_lo; int64_t vt_ld;
    /* Optional caller-owned scratch (fp32, at least 4*M*N floats) for small problems: with few output tiles and a long
     * K the K range is cut into up to 4 slices computed by different blocks, the partial sums go to `workspace` and a
     * second kernel adds them in a fixed order (deterministic) and applies the epilogue.  NULL = never split K.
     * Not available together with the RoPE / QKV-transpose epilogues. */
    float* workspace; int64_t workspace_floats;
    /* Non-zero: the split weight is ONE interleaved matrix [N][K/32][hi 32 | lo 32] (W_lo == W_hi + 32 halves,
     * a->ldw >= 2K halves), so that a K-step of a row is a whole 128-byte cache line.  Large-problem kernel only
     * (pre-split A, M >= 2048, N >= 512). */
    int32_t w_interleaved;
    /* Kernel selection for A/B measurements (0 = default): CVX_GEMM_FLAG_* below.  Results of the kernels agree to fp32
     * rounding.  Other bits are ignored. */
    int32_t flags;
    /* Activation scales: DEVICE pointers to one float each (NULL = 1.0), powers of two.  a_scale_dev = the factor the
     * producer of A_hi/A_lo (and of A2_*: both operands must share it) multiplied the values by before splitting - the
     * accumulators are divided by it (exact); c_scale_dev / vt_scale_dev = the factor applied to the values written to
     * C_hi/C_lo and Vt_hi/Vt_lo (the fp32 store of C is never scaled).  They keep split pairs inside fp16's
     * full-precision window (|x| in [2^-3, 2^16)) whatever the magnitude of the tensor; living in device memory they can
     * be computed by an earlier kernel without a host round trip (and replayed from a captured graph). */
    const float* a_scale_dev; const float* c_scale_dev; const float* vt_scale_dev;
    /* Deferred AdaptiveRMSNorm (version 105; all NULL = off).  The norm between a to_out / ff2 / skip-combiner product and the
     * to_qkv / ff1 product that follows it (acoustic.py:306-318, :198-204) is one gamma / beta row for every frame of an
     * evaluation, so  norm(x) . W^T = (sqrt(D) / ||x_row||) * ((x * gamma) . W^T) + beta . W^T :
     *   the PRODUCER call passes c_gamma_dev ([N] floats: C_hi/C_lo then hold C[m,n] * gamma[n] * *c_scale_dev - the fp32 store of C
     *   is unchanged) and c_rowsq ([M][c_rowsq_ld >= N/64] floats: every 64-column slice of a row leaves its sum of squares there, in
     *   a fixed order); cvx_rownorm_scale_f32 turns those into one factor per row; the CONSUMER call passes them as a_row_scale_dev
     *   ([M] floats, multiplied into row m of the accumulators before bias / activation / RoPE) and beta . W^T as (part of) its bias.
     * No normalised tensor exists in HBM and the norm kernel does not run.  Only the large-problem kernel takes these (pre-split
     * interleaved A and W, M >= 2048, N >= 512, N % 64 == 0, 16-byte aligned epilogue operands) in four forms - producer:
     * residual + fp32 store (to_out, ff2) or A2 + bias + fp32 store (skip combiner); consumer: bias + GELU + split store (ff1) or
     * the QKV mode with an optional bias - and every other combination is refused (CVX_ERR_INVALID). */
    const float* c_gamma_dev; float* c_rowsq; int64_t c_rowsq_ld; const float* a_row_scale_dev;
    /* The residual as a split pair (producer forms with a residual only; a->residual must be NULL): residual[m,n] =
     * (R_hi + R_lo)[m,n] / *r_scale_dev (R_lo == R_hi + 32: interleaved, ldr_h >= 2N).  With write_f32 == 0 the residual stream
     * of the transformer lives in HBM as pairs only - the to_out / ff2 epilogue then moves the bytes the fp32 form moved (read
     * 4 B, write 4 B per element) and the norm kernel's 8 B per element are gone.  c_gamma_dev may be NULL (gamma folded into the
     * consumer's weights instead: cvx_split_f16_colscale_il).  R may alias C_hi / C_lo (same element, same lane). */
    const uint16_t* R_hi; const uint16_t* R_lo; int64_t ldr_h; const float* r_scale_dev;
    /* A | A2 pairs with DIFFERENT pre-scales (skip-combiner producer form only): A2_hi/A2_lo hold a2 * *a2_scale_dev while A holds
     * a * *a_scale_dev (NULL: both operands share a_scale_dev).  Every stage of the pair-only residual stream carries its own
     * power-of-two pre-scale, so a skip saved at the input of layer i and the stream at layer depth-1-i need not share one. */
    const float* a2_scale_dev;
} cvx_gemm_split_io;
/* (bits 1 and 2 selected the two superseded large-problem kernels until version 105: ignored now) */
#define CVX_GEMM_FLAG_MEDIUM 8      /* interleaved operands, 2048 rows and more: take the medium-problem kernel (128 x 128 tiles) whatever the tile count */
#define CVX_GEMM_FLAG_NO_MEDIUM 16  /* ... never take it there (the large-problem kernel's rounds of 256 x 256 tiles): A/B measurements */
#define CVX_GEMM_FLAG_ONE_TILE 4    /* eight-phase 16x16x32 kernel: one output tile per block instead of persistent blocks (bit-identical results) */
#define CVX_GEMM_FLAG_TILE192 64    /* large-problem kernel: 192-row tiles whatever the tile count (default: 192 where rounds x height come out smaller than with 256) */
#define CVX_GEMM_FLAG_TILE256 128   /* ... 256-row tiles always (bit-identical results either way: A/B measurements) */
#define CVX_GEMM_FLAG_TILE_MIXED 32 /* ... whole rounds of 256-row tiles + one launch of 192-row tiles over the rest, wherever such a split exists
                                     * (default: where it is the cheapest of the three; bit-identical results) */
#define CVX_GEMM_FLAG_VT_PIECES 512 /* to_qkv on the eight-phase kernels: the earlier V^T stores (8 bytes per lane, row group by row group) instead of
                                     * line-major 16-byte stores (bit-identical results: the bit-identity test, A/B measurements) */
int cvx_split_f16(const float* w, uint16_t* hi, uint16_t* lo, int64_t n, float scale, cvx_stream_t s);
/* n_sets interleaved split copies of ONE weight matrix with its COLUMNS scaled: out[s][n][il(k)] = split( W[n,k] * colscale[s*cs_ld + k] *
 * set_scale_dev[s*ss_ld] * scale ), each [N][K/32][hi 32 | lo 32] (the w_interleaved layout, row length 2K halves), K % 32 == 0.
 * Deferred AdaptiveRMSNorm with gamma on the weight side: set s = evaluation time s of a solve, colscale = that time's gamma row,
 * set_scale_dev = a power of two that keeps |gamma| <= 1 (the consumer divides it out through a_scale_dev).  W is read once. */
int cvx_split_f16_colscale_il(const float* W, int64_t ldw, int32_t N, int32_t K, const float* colscale, int64_t cs_ld,
                              const float* set_scale_dev, int64_t ss_ld, int32_t n_sets, float scale, uint16_t* out, cvx_stream_t s);
/* the same with an additional DEVICE-resident factor (the pair holds w * scale * *scale_dev; scale_dev may be NULL).
 * An interleaved pair (lo == hi + 32) needs n % 32 == 0: a partial last block of 32 would be stored past 2 * n halves (CVX_EINVAL). */
int cvx_split_f16_dev(const float* w, uint16_t* hi, uint16_t* lo, int64_t n, float scale, const float* scale_dev, cvx_stream_t s);
int cvx_gemm_f16x3(const cvx_gemm_args* a, const uint16_t* W_hi, const uint16_t* W_lo, float acc_scale,
                   const cvx_gemm_split_io* io, cvx_stream_t s);
/* cvx_gemm_f16x3 followed by the AdaptiveRMSNorm / RMSNorm of its fp32 output, as ONE call (reference acoustic.py:306-318: every
 * to_out, ff2 and skip-combiner product of the transformer is followed by the next norm; :198-204, :175):
 *     C = epilogue([A | A2] . W^T)  (fp32, written: io->write_f32 must not be 0, ldc == N, act == NONE);
 *     Y = split( C[r,:] / max(||C[r,:]||_2, eps) * scale * gamma + beta ) * *y_scale_dev     (one gamma / beta row for all rows)
 * Problems that take the split-K path (fewer than 2048 rows, N <= 1024, N % 256 == 0) run the norm inside the split-K reduction
 * (the row is in registers there: no extra launch, no re-read of C); every other problem runs cvx_adarmsnorm_scaled_f32 behind
 * the product.  Both give the same bits. */
typedef struct {
    const float* gamma; const float* beta;          /* [N]; beta may be NULL (RMSNorm) */
    uint16_t* Y_hi; uint16_t* Y_lo; int64_t ldy_h;   /* split pair of the normalised rows, row stride in halves (Y_lo == Y_hi + 32,
                                                      * ldy_h == 2N: interleaved [hi 32 | lo 32]; otherwise ldy_h == N) */
    const float* y_scale_dev;                       /* power-of-two pre-scale of Y in DEVICE memory, NULL = 1 */
    float scale; float eps;                         /* sqrt(N) and 1e-12 in the reference */
} cvx_gemm_norm;
int cvx_gemm_f16x3_norm(const cvx_gemm_args* a, const uint16_t* W_hi, const uint16_t* W_lo, float acc_scale,
                        const cvx_gemm_split_io* io, const cvx_gemm_norm* norm, cvx_stream_t s);
/* Size (in floats) of cvx_gemm_split_io.workspace that lets a problem of this shape split K (0: this shape never does).
 * K1 = the A | A2 boundary of a K-split operand, 0 without A2. */
int64_t cvx_gemm_f16x3_workspace_floats(int32_t M, int32_t N, int32_t K, int32_t K1);

/* y[r,:] = x[r,:] / max(||x[r,:]||_2, eps) * scale * gamma[g,:] + beta[g,:],  g = r / rows_per_group
 * AdaptiveRMSNorm.forward (acoustic.py:198-204) with gamma/beta = the already projected
 * to_gamma/to_beta(time_emb) rows; RMSNorm.forward (:175) when beta == NULL and one group.
 * D % 4 == 0. */
int cvx_adarmsnorm_f32(const float* x, const float* gamma, const float* beta, float* y,
                       uint16_t* y_hi, uint16_t* y_lo,   /* optional fp16 (hi, lo) split copy of y; y may then be NULL */
                       int64_t rows, int32_t D, int64_t rows_per_group, float scale, float eps,
                       cvx_stream_t s);
/* the same; the split copy (y_hi, y_lo) holds y * *split_scale_dev (a power of two in DEVICE memory, NULL = 1: the
 * activation pre-scale of cvx_gemm_split_io.a_scale_dev).  The fp32 output y is never scaled.
 * An interleaved pair (y_lo == y_hi + 32) needs D % 32 == 0: the layout is addressed by flat offset, which is a row's own line of
 * 2 * D halves only then (CVX_EINVAL otherwise; the same holds for cvx_adarmsnorm_f32). */
/* out[r] = scale / max(sqrt(sum_{j < parts} rowsq[r * ld + j]), eps): the per-row factor of a deferred norm from the partial sums a
 * producer GEMM left (cvx_gemm_split_io.c_rowsq; F.normalize's eps clamp, acoustic.py:198-204).  parts <= 64, summed in index order. */
int cvx_rownorm_scale_f32(const float* rowsq, int64_t rows, int32_t parts, int64_t ld, float scale, float eps, float* out, cvx_stream_t s);
int cvx_adarmsnorm_scaled_f32(const float* x, const float* gamma, const float* beta, float* y,
                              uint16_t* y_hi, uint16_t* y_lo,
                              int64_t rows, int32_t D, int64_t rows_per_group, float scale, float eps,
                              const float* split_scale_dev, cvx_stream_t s);

/* out[b,t,h*64+d] = softmax_j( q[b,h,t,:] . k[b,h,j,:] * scale ) @ v[b,h,j,d]
 * Attend.forward non-flash branch (attend.py:108-126) without materialising the T x T
 * scores.  qkv is the to_qkv output [Bt, T, 3*H*64] (q | k | v, heads contiguous
 * 64-blocks, acoustic.py:227-229) with RoPE already applied to q and k (GEMM epilogue).
 * Head dim is fixed at 64 (every shipped config, running_command/Acous_*.sh). */
int cvx_attention_f32(const float* qkv, float* out,
                      uint16_t* out_hi, uint16_t* out_lo,  /* optional fp16 (hi, lo) split copy; out may then be NULL */
                      int32_t Bt, int32_t T, int32_t H, float scale, cvx_stream_t s);

/* ------------------------------------------------------------------------
 * RAGGED BATCHES (utterances of different length in one launch; the reference runs them one at a time,
 * monologue_generation.py:259-304, and its network has no key-padding mask, acoustic.py:313, so an utterance must
 * never see another one).  The n sequences are PACKED: sequence i owns rows [cu_seqlens[i], cu_seqlens[i+1]) of every
 * [M, width] tensor (M = cu_seqlens[n]; cu_seqlens: n+1 int32 in DEVICE memory; max_T = the longest sequence, which
 * sizes the grid).  Everything row-wise (GEMMs, norms, CFG combine, embedding gather) needs nothing; the three
 * operators that look along the time axis take the table:
 *   - attention: keys restricted to the own sequence (the *_varlen entry points below);
 *   - RoPE: run the to_qkv GEMM with rope_T = M and per-ROW tables cos/sin [M][32] (row r: its position inside its
 *     sequence), which also makes its V^T output ONE row set per head over all M columns: vt [H*64, vt_ld],
 *     column = slot(row) - the layout cvx_attention_f16x3_varlen reads (vt_ld >= M rounded up to 32);
 *   - ConvPositionEmbed: zero padding at the ends of every sequence (cvx_dwconv31_gelu_res_varlen_f32).
 * Results per utterance equal its B = 1 run up to fp32 summation order (key tiles stay aligned to 32 packed rows). */
int cvx_attention_varlen_f32(const float* qkv, float* out, uint16_t* out_hi, uint16_t* out_lo,
                             const int32_t* cu_seqlens_dev, int32_t n_seq, int32_t max_T, int32_t H, float scale, cvx_stream_t s);

/* Split-precision variant of cvx_attention_f32 (same reference computation, attend.py:108-126) on
 * v_mfma_f32_32x32x16_f16: inputs are the (fp16 hi, fp16 lo) pairs written by cvx_gemm_f16x3 in QKV mode -
 * qk_* [Bt*T, 2*H*64] (q | k after RoPE) and vt_* [Bt*H*64, Tp] (v transposed per (sequence, head), Tp >= T
 * rounded up to 32, columns >= T finite) - and q.k, p.v are each computed as three fp16 products with fp32
 * accumulation.  Output as for cvx_attention_f32 (fp32 and/or split). */
int cvx_attention_f16x3(const uint16_t* qk_hi, const uint16_t* qk_lo, const uint16_t* vt_hi, const uint16_t* vt_lo,
                        float* out, uint16_t* out_hi, uint16_t* out_lo,
                        int32_t Bt, int32_t T, int32_t Tp, int32_t H, float scale, cvx_stream_t s);
/* the same with activation pre-scales (DEVICE scalars, powers of two, NULL = 1): qk_* hold (q | k) * *qk_scale_dev and
 * vt_* hold v * *v_scale_dev (cvx_gemm_split_io.c_scale_dev / vt_scale_dev of the to_qkv GEMM); both are divided out
 * (the fp32 `out` is the true value) and the split output holds out * *out_scale_dev for the to_out GEMM. */
int cvx_attention_f16x3_scaled(const uint16_t* qk_hi, const uint16_t* qk_lo, const uint16_t* vt_hi, const uint16_t* vt_lo,
                               float* out, uint16_t* out_hi, uint16_t* out_lo,
                               int32_t Bt, int32_t T, int32_t Tp, int32_t H, float scale,
                               const float* qk_scale_dev, const float* v_scale_dev, const float* out_scale_dev, cvx_stream_t s);
/* ragged batch (see RAGGED BATCHES above): qk_* [M, 2*H*64], vt_* [H*64, vt_ld] over all M packed rows */
int cvx_attention_f16x3_varlen(const uint16_t* qk_hi, const uint16_t* qk_lo, const uint16_t* vt_hi, const uint16_t* vt_lo,
                               float* out, uint16_t* out_hi, uint16_t* out_lo, const int32_t* cu_seqlens_dev,
                               int32_t n_seq, int32_t max_T, int64_t M, int32_t vt_ld, int32_t H, float scale,
                               const float* qk_scale_dev, const float* v_scale_dev, const float* out_scale_dev, cvx_stream_t s);

/* Which kernel form cvx_attention_f16x3 / _scaled / _varlen launch for a problem: the launchers take their decision from this
 * very function.  No GPU work, no stream, callable on a machine without a GPU.
 *   n_seq, H: sequences and heads; max_T: frames per sequence (equal-length batch) or the longest sequence (ragged batch);
 *   q_rows: query rows of the launch (n_seq * max_T, or the M packed rows of a ragged batch); single_term != 0: hi halves only.
 * Returns CVX_ATT_FORM_A / _B / _C / _D, plus CVX_ATT_FORM_SINGLE_TERM for the single-term twins, or -1 for arguments no launch
 * can have; writes queries per block, key groups per block and query waves per block where the pointers are not NULL.
 *   D: 256-query blocks of four waves with two query sets each, one key group  (n_seq * H * ceil(max_T / 256) >= 512: the blocks
 *      fill the two slots of every CU at least once; same bits per query as A; three-term launches only)
 *   A: 128-query blocks, one key group  (otherwise: max_T < 128, or 2048 query rows and more)
 *   B: 128-query blocks, three key groups merged through LDS  (otherwise, more than 128 blocks of 128 queries)
 *   C: 64-query blocks of two query waves, four key groups    (otherwise, at most 128 such blocks) */
#define CVX_ATT_FORM_A 0
#define CVX_ATT_FORM_B 1
#define CVX_ATT_FORM_C 2
#define CVX_ATT_FORM_D 3
#define CVX_ATT_FORM_SINGLE_TERM 4
int cvx_attention_f16x3_form(int32_t n_seq, int32_t max_T, int64_t q_rows, int32_t H, int32_t single_term,
                             int32_t* query_block, int32_t* key_groups, int32_t* query_waves);

/* y[b,t,c] = GELU( bias[c] + sum_k w[c,k] * x[b,t+k-K/2,c] ) + x[b,t,c]
 * ConvPositionEmbed + residual (acoustic.py:141-161, :508), channels-last, K == 31. */
int cvx_dwconv31_gelu_res_f32(const float* x, const float* w, const float* bias, float* y,
                              int32_t Bt, int32_t T, int32_t C, cvx_stream_t s);
/* ragged batch (see RAGGED BATCHES above): x, y [M, C] packed */
int cvx_dwconv31_gelu_res_varlen_f32(const float* x, const float* w, const float* bias, float* y,
                                     const int32_t* cu_seqlens_dev, int32_t n_seq, int32_t max_T, int32_t C, cvx_stream_t s);
/* C[M][N] = act(A[M][K] . W[N][K]^T + bias) for a HANDFUL of rows (M <= 32, K % 8 == 0; round 3): weight streaming - every W row
 * is read once (non-temporal) by one wave and multiplied with all rows of A from LDS; exact fp32 FMAs.  The adaptive-norm
 * table of a solve (acoustic.py:360-370 evaluated for all n evaluation times at once: 32 x 32,768 x 1,024) and the time MLP. */
int cvx_gemm_skinny_f32(const float* A, int32_t lda, const float* W, int64_t ldw, const float* bias, float* C, int64_t ldc,
                        int32_t M, int32_t N, int32_t K, int32_t act, cvx_stream_t s);
/* v = f_c*(1+s) - s*f_n   (f_n == NULL: v = f_c)        CFG combine, acoustic.py:428
 * out = y + coef*v ; out2, out3 = optional extra copies  ODE stage update (torchdiffeq midpoint:
 * y_mid = y + f0*dt/2, y1 = y + dt*f_mid); `out` may alias `y`. */
int cvx_cfg_combine_axpy_f32(const float* f_c, const float* f_n, const float* y, float cond_scale,
                             float coef, float* out, float* out2, float* out3, int64_t n, cvx_stream_t s);
/* CFG combine + one stage of an explicit Runge-Kutta step (fixed grid, at most 4 stages), one launch per field evaluation.
 * Per element i of rows x dim (all tensors contiguous [rows, dim]):
 *   v = f_c[i]
 *   f_n != NULL:  s = row_scale ? row_scale[i / dim] : cond_scale ;  unless (row_scale && s == 1.0f):  v = v*(1+s) - s*f_n[i]
 *   k_out != NULL: k_out[i] = v                                   (the combined field of this stage, kept for later stages)
 *   o = y[i] ;  for j = 0 .. m-1 with w[j] != 0:  o += k_prev[j][i] * w[j] ;  if w[m] != 0:  o += v * w[m]
 *   out[i] = o ;  out2, out3 = optional extra copies ;  `out` may alias `y`
 * k_prev: HOST array of m device pointers (m <= 3), w: HOST array of m + 1 floats - the caller's fp32(dt * a_ji), or fp32(dt * b_j)
 * on the last stage of a step.  A stage whose weight is exactly 0 is neither read nor added (its pointer may be NULL).
 * row_scale: one guidance scale per ROW on the device (needs f_n); a row at exactly 1.0 takes f_c - the reference's branch
 * (acoustic.py:423), which the formula does not reach continuously.  With m == 0, k_out == NULL and row_scale == NULL the result has
 * the bits of cvx_cfg_combine_axpy_f32 with coef = w[0].  16-byte accesses when every pointer is 16-byte aligned.
 * CVX_EINVAL, nothing launched: NULL f_c / y / out / w, m outside 0..3, NULL k_prev[j] with w[j] != 0, rows < 0, dim <= 0,
 * row_scale without f_n. */
int cvx_rk_stage_f32(const float* f_c, const float* f_n, const float* y, float cond_scale, const float* row_scale,
                     const float* const* k_prev, const float* w, int32_t m, float* k_out, float* out, float* out2, float* out3,
                     int64_t rows, int32_t dim, cvx_stream_t s);
/* The LAST stage of a step with the embedded error estimate.  Everything cvx_rk_stage_f32 does - out, out2, out3 and k_out have that
 * kernel's bits for the same arguments - plus, per element, with v the combined field and o the new state of this launch:
 *   delta = 0 ;  for j = 0 .. m-1 with we[j] != 0:  delta = fma(k_prev[j][i], we[j], delta) ;  if we[m] != 0:  delta = fma(v, we[m], delta)
 * we: HOST array of m + 1 floats, the caller's fp32(dt * (b_j - b_err_j)): delta is the local error of the lower-order solution on
 * the same stages.  A stage whose w[j] is 0 and whose we[j] is not must still be given (midpoint's k_0).
 * A block owns one chunk of at most CVX_RK_ERR_ROWS consecutive rows of ONE sequence, counted from that sequence's first row (the
 * last chunk of a sequence is short), and writes partials[block] = (sum delta^2, sum o^2) over its chunk: per-thread sums in element
 * order, 64-lane butterfly, the four waves in wave order through LDS - no atomics, a function of the chunk's own rows only.
 * map_dev: DEVICE int32 [blocks][3] = (first row, rows, sequence) per block; map_host: the same table on the HOST, checked here:
 * the chunks must tile [0, rows) in order, 1 .. CVX_RK_ERR_ROWS rows each, sequences ascending, a short chunk ending its sequence.
 * partials: DEVICE float [blocks][2] of this step, 8-byte aligned.  16-byte accesses when every pointer is 16-byte aligned and
 * dim % 4 == 0 (every chunk then starts on a 16-byte boundary), 4-byte accesses otherwise; the sums may differ between the two forms.
 * CVX_EINVAL, nothing launched: whatever cvx_rk_stage_f32 refuses; NULL we, map_dev, map_host or partials; NULL k_prev[j] with
 * we[j] != 0; a map that does not tile the launch's rows as described. */
#define CVX_RK_ERR_ROWS 32
int cvx_rk_stage_err_f32(const float* f_c, const float* f_n, const float* y, float cond_scale, const float* row_scale,
                         const float* const* k_prev, const float* w, const float* we, int32_t m, float* k_out, float* out, float* out2,
                         float* out3, int64_t rows, int32_t dim, const int32_t* map_dev, const int32_t* map_host, int32_t blocks,
                         float* partials, cvx_stream_t s);
/* err[step][q] = (sum delta^2, sum o^2) of sequence q at every step: the partials [steps][blocks][2] of the blocks the map gives to
 * q, added in block order by one thread.  One launch at the end of a solve.  err: DEVICE float [steps][n_seq][2], 8-byte aligned. */
int cvx_rk_err_finish_f32(const float* partials, const int32_t* map_dev, int32_t blocks, int32_t steps, int32_t n_seq, float* err,
                          cvx_stream_t s);

/* rows of [ emb(ids[m,0]) | emb(ids[m,1]) ... | cond[m,:] ]  -> out[M, S*E + Cc]
 * (the step-invariant columns of the to_embed input, acoustic.py:496-503).
 * ids == NULL: every id is `null_id`; cond_row != NULL: cond is that single broadcast row
 * (CFG null substitution, acoustic.py:473-494). */
int cvx_embed_gather_f32(const int64_t* ids, int32_t S, const float* table, int32_t E, int32_t n_rows_table,
                         const float* cond, const float* cond_row, int32_t Cc, int64_t null_id,
                         float* out, int64_t M, cvx_stream_t s);

/* out[i, :] = cat( sin(t_i * w * 2pi), cos(t_i * w * 2pi) )   LearnedSinusoidalPosEmb (acoustic.py:107-111) */
int cvx_time_fourier_f32(const float* times, const float* w, float* out, int32_t n, int32_t half,
                         cvx_stream_t s);

/* ------------------------------------------------------------------------
 * HiFi-GAN generator (covomix/vocoder/models.py:75-125, hifi-gan/config_covomix.json)
 *
 * One implicit-GEMM fp32-MFMA kernel covers Conv1d (dilated, "same" padding) and
 * ConvTranspose1d (as a stride-1 conv over the zero-stuffed input with the flipped
 * kernel):  out[b,co,l] = ((bias[co] + sum_{ci,kk} Wp[co,ci,kk] * z[b,ci,l + kk*dil - pad]
 *                          + res[b,co,l]) + accum[b,co,l]) * out_scale
 *   z = leaky_relu(x, in_slope) zero-stuffed by `up` (up == 1: plain conv), zero outside.
 * Wp is the packed weight produced by cvx_hifigan_pack_weight_f32 (host-side layout
 * [co_blk][ci_chunk][kk][CO_T][16]).  res / accum may be NULL; accum may alias out.
 * Covers conv_pre (:81), ups[i] preceded by leaky_relu (:102-103), every ResBlock1
 * conv with its preceding leaky_relu and residual add (:35-42) and the
 * xs accumulate / divide by num_kernels (:104-110). */
/* Ragged batches in the vocoder (items of different length in one launch; the reference vocodes utterances one by
 * one, monologue_generation.py:52-59, :299-304): all tensors are sized for the LONGEST item and item b is valid on its
 * first  item_len_dev[b] * mul + add  OUTPUT positions (the lengths of a stage are an affine function of the item's
 * mel frames: item_len_dev holds the frames, the caller supplies the stage's mul / add).  A kernel given this table
 * writes ZEROS behind an item's last valid position (up to the common length), which is exactly the zero padding the
 * next convolution of a B = 1 run sees there; inputs must obey the same rule (zero-padded mel).  item_len_dev == NULL:
 * every item has the common length.
 * `accum` (and `res`) are INPUTS under that rule: they must hold zeros behind an item's end, as every buffer one of these kernels
 * wrote with the same table does.  With a non-zero accum there the kernels differ, and none of it is a promise:
 *   cvx_hifigan_conv1d_f32, cvx_hifigan_resblock_pair_f16x3 (and the narrow stages of cvx_hifigan_resblock_*_f16x3): zero after the
 *     accumulate - out is zero behind the end whatever accum holds there;
 *   cvx_hifigan_conv1d_f16x3 / _group_ (and the wide stages of cvx_hifigan_resblock_*_f16x3): zero BEFORE the accumulate -
 *     out_x = accum * out_scale behind the end (out_zhi / out_zlo are zero: they never see accum);
 *   a non-zero res behind the end is dropped by all of them.
 * The clamps: an item's length is min(common length, max(0, item_len_dev[b] * mul + add)). */
typedef struct { const int32_t* item_len_dev; int32_t mul, add; } cvx_item_lengths;
typedef struct {
    const float* x;  int32_t B, Cin, Lin;
    const float* Wp; const float* bias;
    float* out;      int32_t Cout, Lout;
    int32_t ksize, dil, pad, up;
    float in_slope;
    const float* res; const float* accum; float out_scale;
    cvx_item_lengths items;                      /* ragged batch (valid OUTPUT positions per item) or {NULL, 0, 0} */
} cvx_conv_args;
int     cvx_hifigan_conv1d_f32(const cvx_conv_args* a, cvx_stream_t s);
/* number of floats of the packed weight for (Cout, Cin, ksize) */
int64_t cvx_hifigan_packed_weight_floats(int32_t Cout, int32_t Cin, int32_t ksize);
/* host-side (CPU) packing of a Conv1d weight [Cout,Cin,k] (transposed == 0) or a
 * ConvTranspose1d weight [Cin,Cout,k] (transposed != 0, kernel flipped) into Wp. */
int     cvx_hifigan_pack_weight_f32(const float* w, int32_t Cout, int32_t Cin, int32_t ksize,
                                    int32_t transposed, float* Wp);

/* ConvTranspose1d (models.py:85-88, :102-103: leaky_relu then ups[i]) in POLYPHASE form: output l = stride*m + r only sees the
 * taps kk = kk0 + stride*j of the flipped kernel, so every phase r is a stride-1 convolution with ceil((k - kk0)/stride) taps
 * over the input as it is - 1/stride of the matrix work of the zero-stuffed form (cvx_hifigan_conv1d_f32 with up > 1, which
 * stays as the cross-check).  `a` is read exactly like cvx_hifigan_conv1d_f32 reads it for that form (up = stride, dil = 1,
 * pad = ksize - 1 - padding, Lout = (Lin-1)*up + 1 + 2*pad - (ksize-1); no res / accum) except that a->Wp is the phase-major
 * packed weight written by cvx_hifigan_pack_conv_transpose1d_f32 (w = the module's [Cin, Cout, k] weight, pad_t = its padding;
 * cvx_hifigan_conv_transpose1d_packed_floats floats).  amax_bits_dev (optional, DEVICE uint32, zero before the call): the
 * launch leaves the bit pattern of max|out| there - cvx_pow2_scale_from_amax_f32 turns it into the next stage's
 * activation pre-scale (as cvx_amax_pow2_scale_f32 would from a separate pass over out) and zeroes it again. */
int     cvx_hifigan_conv_transpose1d_f32(const cvx_conv_args* a, uint32_t* amax_bits_dev, cvx_stream_t s);
int64_t cvx_hifigan_conv_transpose1d_packed_floats(int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, int32_t pad_t);
int     cvx_hifigan_pack_conv_transpose1d_f32(const float* w, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride,
                                              int32_t pad_t, float* Wp);
int     cvx_pow2_scale_from_amax_f32(uint32_t* amax_bits_dev, float target, float* scale_dev, cvx_stream_t s);

/* y[b,0,l] = tanh( bias + sum_{ci,k} w[ci,k] * leaky_relu(x[b,ci,l+k-3], slope) )
 * final leaky_relu (default slope 0.01, models.py:112) + conv_post + tanh (:113-114). ksize == 7. */
int cvx_hifigan_post_f32(const float* x, const float* w, float bias, float* y,
                         int32_t B, int32_t Cin, int32_t L, float slope, cvx_stream_t s);

/* ------------------------------------------------------------------------
 * ResBlock1 convolutions (covomix/vocoder/models.py:11-48, 97 % of the vocoder's FLOPs) on the fp16 matrix pipe
 * with split-precision operands (three v_mfma_f32_32x32x16_f16 per product, fp32 accumulate - same scheme and
 * accuracy class as cvx_gemm_f16x3).  Stride-1 "same" convolution, pad = (ksize-1)*dil/2 (utils.py:34-35).
 *
 * All tensors here are CHANNELS-LAST with zero halos: [B][Lp][Cp], position l of batch b at row b*Lp + halo_l + l,
 * rows outside [halo_l, halo_l + L) and channels >= C must hold zeros (the kernels keep them zero);
 * halo_l >= pad, Lp >= halo_l + roundup(L, 256) + 64, Cp = channels rounded up to a multiple of 32.
 *   z_hi/z_lo : input = leaky_relu of the previous value, as (fp16 hi, fp16 lo) pairs, [B][Lp][Cp_in]
 *   w_hi/w_lo : weights pre-scaled by 1/acc_scale and split, packed [Cp_in/32][ksize][Np][32 ci]
 *   v = acc*acc_scale + bias[co] (+ res);   out_x = (v (+ accum)) * out_scale   [fp32, optional]
 *   out_zhi/out_zlo = split(leaky_relu(v, z_slope))                             [optional: the next conv's input]
 * Np (padded output channels) must be 32, 64, 128 or 256; (ksize-1)*dil even and <= 50.
 */
typedef struct {
    const uint16_t *z_hi, *z_lo;
    int32_t B, L, Lp, Cp_in, halo_l;
    const uint16_t *w_hi, *w_lo;
    float acc_scale;
    const float* bias;
    int32_t Np, ksize, dil;
    const float* res;
    const float* accum;
    float* out_x;
    float out_scale;
    uint16_t *out_zhi, *out_zlo;
    float z_slope;
    /* Activation pre-scale of this ResBlock stage (DEVICE scalar, power of two, NULL = 1): z_hi/z_lo hold
     * leaky_relu(x) * *z_scale_dev (the accumulators are divided by it, exactly) and out_zhi/out_zlo are written times
     * it; res / accum / out_x are true fp32 values.  Keeps the split pairs inside fp16's full-precision window whatever
     * the magnitude of the stage's activations (cvx_amax_pow2_scale_f32 measures it from the stage input). */
    const float* z_scale_dev;
    cvx_item_lengths items;                      /* ragged batch (valid positions per item, of L) or {NULL, 0, 0} */
} cvx_conv16_args;
int cvx_hifigan_conv1d_f16x3(const cvx_conv16_args* a, cvx_stream_t s);
/* n (1..3) INDEPENDENT convolutions of one shape (B, L, Lp, Cp_in, Np, halo_l, items; kernel size, dilation, weights, inputs and outputs their
 * own; outputs must not alias) as ONE launch: the same results as n calls above, bit for bit - the tiles of the short kernels fill the rounds
 * of the long one (round 6: the three ResBlocks of a generator stage, kernel sizes 3 / 7 / 11, models.py:104-110). */
int cvx_hifigan_conv1d_group_f16x3(const cvx_conv16_args* a, int32_t n, cvx_stream_t s);
/* Positions per thread block (the tile height: 256, 192 or 160 rows) of the launch the two calls above make for n_problems (1..3; the
 * column tiles of a conv-transpose: up to 8) convolutions of Np output columns, L positions and B items on a context of `cus` compute
 * units (> 0): 256 for Np <= 128; for Np = 256 the height whose rounds x height is smallest (192-row blocks where they need fewer
 * rounds, 160-row blocks of the 16x16x32 kernel where they beat both at 1.13 x their cost).  The launcher calls the same function.
 * Host arithmetic only - no device work; -1 for arguments no launch has. */
int cvx_hifigan_conv1d_f16x3_form(int32_t Np, int32_t L, int32_t B, int32_t n_problems, int32_t cus);

/* ResBlock1.forward (covomix/vocoder/models.py:35-42) on the split-precision convolution above - the operator-level
 * form of section 8(b)'s cvx_hifigan_resblock_* for the path the host actually runs: three times
 *     x = c2(leaky_relu(c1(leaky_relu(x, .1)), .1)) + x        (c1: dilation dil[m], c2: dilation 1)
 * on channels-last buffers [B][Lp][Np] (layout rules of cvx_conv16_args; Np = the stage's padded channel count for
 * inputs and outputs).  x (fp32) and z = split(leaky_relu(x) * *z_scale_dev) are the block's input and are not
 * modified; t, xa/za, xb/zb are caller-owned scratch of the same shapes (xa/za, xb/zb alternate as the intermediate
 * x / z of the pairs).  The last pair writes out = (x_final (+ accum)) * out_scale (accum may alias out): the
 * generator's xs (+)= resblock(x), / num_kernels on the last block (models.py:104-110).  Six launches. */
typedef struct {
    const uint16_t *w_hi, *w_lo; float acc_scale; const float* bias;     /* one convolution: cvx_conv16_args fields */
} cvx_conv16_weights;
typedef struct {
    const float* x; const uint16_t *z_hi, *z_lo;
    int32_t B, L, Lp, Np, halo_l;
    cvx_conv16_weights c1[3], c2[3];
    int32_t ksize; int32_t dil[3];
    uint16_t *t_hi, *t_lo;
    float* xa; uint16_t *za_hi, *za_lo;
    float* xb; uint16_t *zb_hi, *zb_lo;
    const float* accum; float* out; float out_scale;
    const float* z_scale_dev;
    cvx_item_lengths items;                      /* ragged batch (valid positions per item, of L) or {NULL, 0, 0} */
} cvx_resblock16_args;
int cvx_hifigan_resblock_f16x3(const cvx_resblock16_args* a, cvx_stream_t s);
/* The n (1..3) ResBlocks of ONE generator stage (models.py:104-110: xs = sum_j resblocks[j](x), / num_kernels): the results of
 * cvx_hifigan_resblock_f16x3(&blocks[0]) ... (&blocks[n-1]), bit for bit, with the convolutions of different blocks that do not depend on
 * each other sharing launches (cvx_hifigan_conv1d_group_f16x3; 18 -> 8 launches on a wide stage).  The blocks name the same x / z / shape, their
 * OWN scratch (t, xa/za, xb/zb) and may share `out`, which their last convolutions accumulate into in block order (blocks[j].accum = out for
 * j > 0).  Blocks that do not qualify (narrow stages: fused pair kernels; shared scratch) run one after the other. */
int cvx_hifigan_resblock_stage_f16x3(const cvx_resblock16_args* blocks, int32_t n, cvx_stream_t s);

/* One ResBlock1 pair  out = (c2(leaky_relu(c1(leaky_relu(x, .1)), .1)) + x (+ accum)) * out_scale  (models.py:36-40; c1:
 * dilation dil, c2: dilation 1, both kernel size ksize) as ONE kernel for the narrow stages (Np = 32 or 64): the
 * intermediate activation stays in LDS and no split pair exists in HBM - the launch reads x (with a halo) and writes
 * out.  x / accum / out: fp32 channels-last [B][Lp][Np] with the layout rules of cvx_conv16_args, and at least
 * (ksize-1)*(dil+1)/2 zero rows on either side of the signal; out must not alias x (accum may alias out).
 * *z_scale_dev (power of two, NULL = 1) is the pre-scale the in-kernel split pairs of leaky_relu(x) and of the
 * intermediate carry.  cvx_hifigan_resblock_f16x3 uses it for Np <= 64 (its z / t / za / zb buffers may then be NULL). */
typedef struct {
    const float* x;
    int32_t B, L, Lp, Np, halo_l;
    cvx_conv16_weights c1, c2;
    int32_t ksize, dil;
    const float* accum; float* out; float out_scale;
    const float* z_scale_dev;
    int32_t flags;      /* 0; bit 0 (dev A/B): Np = 64 on 128-row tiles, two blocks per CU, instead of 256-row tiles, one per CU */
    cvx_item_lengths items;                      /* ragged batch (valid positions per item, of L) or {NULL, 0, 0} */
} cvx_respair16_args;
int cvx_hifigan_resblock_pair_f16x3(const cvx_respair16_args* a, cvx_stream_t s);

/* Layout converters between the channel-major fp32 tensors of cvx_hifigan_conv1d_f32 ([B][C][L]) and the
 * channels-last buffers above: to_channels_last writes the fp32 copy (x_cl, optional) and / or the split pair of
 * leaky_relu(x, slope) (z_hi/z_lo, optional); from_channels_last the reverse of the fp32 copy. */
int cvx_hifigan_to_channels_last(const float* x, float* x_cl, uint16_t* z_hi, uint16_t* z_lo, int32_t B, int32_t C,
                                 int32_t L, int32_t Lp, int32_t Cp, int32_t halo_l, float slope, cvx_stream_t s);
int cvx_hifigan_to_channels_last_scaled(const float* x, float* x_cl, uint16_t* z_hi, uint16_t* z_lo, int32_t B, int32_t C,
                                        int32_t L, int32_t Lp, int32_t Cp, int32_t halo_l, float slope,
                                        const float* z_scale_dev /* the pair holds leaky_relu(x) * *z_scale_dev; NULL = 1 */,
                                        cvx_stream_t s);
int cvx_hifigan_from_channels_last(const float* x_cl, float* x, int32_t B, int32_t C, int32_t L, int32_t Lp,
                                   int32_t Cp, int32_t halo_l, cvx_stream_t s);
/* leaky_relu + ConvTranspose1d (the upsamplers, covomix/vocoder/models.py:85-88, :102-103) on the split-precision pipe,
 * channels-last in and out (round 3; the fp32 form is cvx_hifigan_conv_transpose1d_f32, channel-major).
 * Stride-1 form: output position stride * m + r only sees the kernel taps c_r + stride * j (c_r = (r + padding) mod stride) at the inputs m + a_r - j
 * (a_r = (r + padding) div stride): the layer is ONE stride-1 convolution over the input with stride * Np_out output
 * columns - column r * Np_out + co of row m is channel co of position stride * m + r, which is exactly the channels-last
 * output buffer read as rows of `stride` positions.  The columns are cut into n_tiles tiles of tile_np (a whole number of
 * phases); tile t runs tile_taps[t] taps, tap kk reading input row m + kk - tile_pad[t], from the packed weights at
 * w_hi/w_lo + tile_w_off[t] (layout [Cp_in/32][tile_taps[t]][tile_np][32 ci], pre-scaled by 1/acc_scale and split, taps a
 * phase does not see are zero).  covomix_amd.ops.hifigan_pack_conv_transpose1d_f16x3 builds weights, bias and table.
 *   z_hi/z_lo : split(leaky_relu(x) * *z_scale_dev) of the input, [B][Lp_in][Cp_in], layout rules of cvx_conv16_args
 *   bias      : [stride * Np_out], bias[co] repeated per phase (zero in the padded channels)
 *   out       : fp32 [B][Lp_out][Np_out], rows halo_out + l for l < L_out = (L_in - 1) * stride + kernel size - 2 * padding are
 *               written (zeros behind an item's end when `items` - lengths in OUTPUT positions - is set); rows m >= L_in of
 *               the stride-1 form (config_covomix's first upsampler: L_out = 5 L_in + 1) read the zero rows behind the input:
 *               ceil(L_out / stride) <= L_in + 32; Lp_out >= halo_out + L_out
 *   amax_bits_dev : optional; receives the bit pattern of max |out| (atomicMax; feed cvx_pow2_scale_from_amax_f32) */
typedef struct {
    const uint16_t *z_hi, *z_lo;
    int32_t B, L_in, Lp_in, Cp_in, halo_in;
    const uint16_t *w_hi, *w_lo;
    float acc_scale;
    const float* bias;
    int32_t Np_out, stride, n_tiles, tile_np;
    int32_t tile_taps[8], tile_pad[8];
    int64_t tile_w_off[8];                       /* in halves */
    float* out;
    int32_t L_out, Lp_out, halo_out;
    const float* z_scale_dev;
    uint32_t* amax_bits_dev;
    cvx_item_lengths items;
} cvx_convt16_args;
int cvx_hifigan_conv_transpose1d_f16x3(const cvx_convt16_args* a, cvx_stream_t s);
/* z = split(leaky_relu(x, slope) * *z_scale_dev) over n floats of a channels-last fp32 buffer (n % 4 == 0; the whole
 * buffer: zero rows and channels stay zero) - the input pair of the call above / of cvx_hifigan_conv1d_f16x3. */
int cvx_hifigan_split_channels_last(const float* x_cl, uint16_t* z_hi, uint16_t* z_lo, int64_t n, float slope,
                                    const float* z_scale_dev, cvx_stream_t s);
/* cvx_hifigan_post_f32 (leaky_relu + conv_post + tanh, models.py:112-114) reading the channels-last stage output
 * [B][Lp][Np] (Np <= 64, halo_l >= 3, zero rows around the signal): same summation order, same bits. y: [B][L]. */
int cvx_hifigan_post_channels_last_f32(const float* x_cl, const float* w, float bias, float* y, int32_t B, int32_t C, int32_t Np,
                                       int32_t L, int32_t Lp, int32_t halo_l, float slope, cvx_stream_t s);
/* *scale_dev = 2^round(log2(target / max|x|)) (1 when x is all zero; exponent clamped to +-40): the power-of-two factor that
 * brings the largest magnitude of x to about `target`.  Everything stays on the device (scratch_dev: one uint32 of
 * caller-owned scratch, any value before the call, ZERO after it - so the same word can serve as a producer's amax_bits_dev
 * next), so a consumer kernel can use the scale without a host round trip. */
int cvx_amax_pow2_scale_f32(const float* x, int64_t n, float target, float* scale_dev, uint32_t* scratch_dev, cvx_stream_t s);

/* ------------------------------------------------------------------------
 * Prompt mel extraction - SURVEY.md section 8f row N3 (data_preparation/generate_mel.py:49-72 as called by
 * monologue_generation.py:62-74): the 480-point windowed DFT of every frame and the mel projection are two calls of
 * cvx_gemm_bias_act_f32 (A = the reflect-padded signal viewed as overlapping rows, lda = hop = 160; W = the
 * hann-windowed cos | sin basis [482, 480]; then the [80, 244] mel basis); these two are the steps in between:
 *   mag[t, k] = sqrt(re[t,k]^2 + im[t,k]^2 + 1e-9)  for k < nb (= 241), 0 for nb <= k < nbp      spec = [T, 2*nb] (re | im)
 *   y[m, t]   = log(max(x[t, m], 1e-5))                                                         x = [T, n_mels]
 */
int cvx_mel_magnitude_f32(const float* spec, float* mag, int64_t T, int32_t nb, int32_t nbp, cvx_stream_t s);
int cvx_mel_log_transpose_f32(const float* x, float* y, int64_t T, int32_t n_mels, cvx_stream_t s);

/* MANY PROMPTS IN ONE CALL (ragged batch; opt-in - the two entry points above and the one-prompt path built on them are unchanged).
 * Geometry: n_fft % 4 == 0, hop % 4 == 0, hop <= n_fft, (n_fft - hop) % 2 == 0, pad = (n_fft - hop) / 2, window = n_fft, no centring.
 * The prompts are PACKED into one buffer of reflect-padded signals: item b has n_b samples at the target rate (n_b = n_raw for a stored
 * signal, ceil(up * n_raw / down) for one that names a resample bank), its padded signal of n_b + 2 * pad samples starts at float
 * S_b = slot_b * hop and takes ceil((n_b + 2 * pad) / hop) hop-sized slots; the next item starts at the next slot; the slack behind an
 * item and the n_fft - hop floats behind the last slot are ZERO.  Frame t of item b is row slot_b + t of ONE [R, n_fft] view with row
 * stride hop over the whole buffer (R = all slots), T_b = (n_b + 2 * pad - n_fft) / hop + 1 frames (0 when the padded item is shorter
 * than n_fft).  A valid row reads only its own item's padded samples; the rows that straddle into the next item are computed and never
 * gathered.  The DFT and the mel projection are then ONE fp32 GEMM each over all R rows, and an item's mel is bit for bit what the
 * one-prompt path gives it alone (every form of the fp32 GEMM contracts an element's products in one order whatever M is).
 *
 * ITEM TABLE: int32 words, filled on the HOST by cvx_mel_items_fill (cvx_mel_items_words of them); the caller uploads a copy and
 * passes both with their word count.
 *   header[16]      magic, n_items, n_fft, hop, pad, R, M = sum T_b, max T_b, packed floats (R * hop + n_fft - hop, rounded up to 4),
 *                   raw floats, n_banks, bank floats, 0 ...
 *   item[n][8]      raw offset (floats into `raw`: the items' stored samples one after the other, every start rounded up to 4), n_raw,
 *                   n_b, slot_b, T_b, cu_b (frames of the items before), bank (-1: none), 0
 *   bank[n_banks][4]  up, down, width, offset (floats into `banks`) of a polyphase filter bank [up][2 * width + down] as
 *                   cvx_resample_fir_f32 takes it (covomix_amd.hubert.sinc_resample_kernel); the banks lie one after the other
 * bank_geom = n_banks triples (up, down, width) in host memory, at most 16 banks.  cvx_mel_items_fill returns CVX_EINVAL and
 * cvx_mel_items_words -1 (nothing is launched, here and in every call that takes a table) when n_items <= 0, the geometry breaks the
 * constraints above, an item has n_b <= pad (its reflection is undefined), names no bank of the call or has n_raw < 0, or the packed
 * buffer, the raw samples or the banks do not fit int32 or the frames reach 2^24.  T_b = 0 is legal.
 * Every call that takes a table re-derives the host copy from its own n_raw / bank words and compares it word by word, then reads the
 * device copy back (one small blocking copy on the context's stream: these calls are NOT graph-capturable) and compares it with the
 * host copy - before anything is launched.  Nothing is allocated and nothing is copied from the host.
 *
 * cvx_mel_pack_f32: ONE launch writes every word of packed[header[8]]: position p of item b takes the stored sample at the reflected
 * index of p - pad, or - for an item with a bank - the polyphase FIR output at that index (the loop of cvx_resample_fir_f32: same taps,
 * same fmaf order, zero outside [0, n_raw)), clamped to [-1, 1]; slack and tail are written as zero.  raw and packed 16-byte aligned.
 * cvx_mel_log_gather_f32: out[n_mels * cu_b + m * T_b + t] = log(max(proj[(slot_b + t) * n_mels + m], 1e-5)): item b's [n_mels, T_b]
 * block is contiguous in the packed output of n_mels * M floats; proj = [R, n_mels].
 * cvx_mel_spectrogram_many_f32: the whole call - pack, DFT GEMM (A = the packed buffer, lda = hop; dft = [2 * nb, n_fft], the windowed
 * cos | sin basis, nb = n_fft / 2 + 1), cvx_mel_magnitude_f32, mel GEMM (basis = [n_mels, nbp], nbp = nb rounded up to 4, zero in the
 * padding), log-gather.  workspace: 256-byte aligned device memory of cvx_mel_workspace_bytes_many bytes (-1 for an illegal table); it
 * needs no initialisation - every word that is read was written by the call. */
int64_t cvx_mel_items_words(int32_t n_fft, int32_t hop, const int64_t* n_raw, const int32_t* bank, const int32_t* bank_geom,
                            int32_t n_banks, int32_t n_items);
int cvx_mel_items_fill(int32_t n_fft, int32_t hop, const int64_t* n_raw, const int32_t* bank, const int32_t* bank_geom, int32_t n_banks,
                       int32_t n_items, int32_t* table, int64_t table_words);
int cvx_mel_pack_f32(const float* raw, const float* banks, const int32_t* items_host, const int32_t* items_dev, int64_t items_words,
                     int32_t n_items, float* packed, cvx_stream_t s);
int cvx_mel_log_gather_f32(const float* proj, const int32_t* items_host, const int32_t* items_dev, int64_t items_words, int32_t n_items,
                           int32_t n_mels, float* out, cvx_stream_t s);
int64_t cvx_mel_workspace_bytes_many(const int32_t* items_host, int64_t items_words, int32_t n_items, int32_t n_mels);
int cvx_mel_spectrogram_many_f32(const float* raw, const float* banks, const float* dft, const float* basis, int32_t n_mels,
                                 const int32_t* items_host, const int32_t* items_dev, int64_t items_words, int32_t n_items,
                                 float* out, void* workspace, int64_t workspace_bytes, cvx_stream_t s);

/* pcm[i] = (int16) trunc( wav[i] * 32768 )   mel_decode_to_wav tail (monologue_generation.py:55-57),
 * numpy astype('int16') semantics for in-range values (C truncation toward zero). */
int cvx_wav_to_int16(const float* wav, int16_t* pcm, int64_t n, cvx_stream_t s);

/* ------------------------------------------------------------------------
 * text2semantic autoregressive decode - SURVEY.md section 8f row N1 ("next" row, built after the hot path).
 *
 * cvx_t2s_decode_steps enqueues n_steps token steps of the sampling loop of TextToSemantic.generate
 * (covomix/covomix_model/text2semantic.py:748-820) at batch 1 with a KV cache: per decoder layer
 * Attention.forward for the causal self-attention (:225-270, rotary_embedding_torch.py:146-157) and the
 * cross-attention over [learned null k/v | encoder context] (:253-262), the GEGLU FeedForward (:154-167), then
 * final RMSNorm (:143-151), tied logits (:545), top_k (:126-132) or top_p (:118-124) + gumbel_sample (:105-113) from the caller's
 * U(0,1) draws, eos bookkeeping (:803-818) and the embedding of the sampled ids as the next input.
 * No host synchronisation: positions live in the slot records on the device, so a captured graph replays.
 *
 * Host packing contract (neurips2024-covomix_amd/t2s.py):
 *   wqkv_s [3*inner, dim] = to_q | to_k | to_v rows; inside every 64-row head of to_q and to_k the rows are
 *       permuted (0,2,..,62,1,3,..,63) so the reference's interleaved rotary pairs become half-split pairs;
 *   kv_c   [dialogues, ctx_rows, 2, inner]: row 0 = null_kv, rows 1.. = to_kv(encoder output), computed once per dialogue
 *       (dialogue = utterance; without a queue dialogue b is decoded by slot b);
 *   k_cache / v_cache [slots, max_len, inner]; every per-slot buffer below is [slots, ...] with slots = batch for batch in
 *       {1, 2, 4} and batch rounded up to a multiple of 8 otherwise (the kernels work on groups of 8 slots);
 *   w2     [dim, ff_inner_pad]: the K dimension zero-padded to a multiple of 4;
 *   rope_cos / rope_sin [max_len, 32]: cos / sin(position * freqs[i]);
 *   uniforms [dialogues, uniform_steps, streams, vocab]; tokens [dialogues, streams, max_len] int64;
 *   batch (1..64) slots advance together, EACH AT ITS OWN POSITION; a weight row is read once per step and group of 8
 *   slots, and the arithmetic per utterance does not depend on the batch size, the slot or the other slots' positions
 *   (results are bit-identical to batch 1);
 *   state int32[slots][8] (slot records): [0] position (= tokens produced so far), [1] 1 once an eos was sampled in any
 *       stream, [2] number of steps at that moment, [3] context rows (null row included) used when n_ctx == 0, so that one
 *       captured graph serves utterances of different text length, [4] the dialogue the slot decodes (indexes kv_c, uniforms,
 *       tokens; the caller writes the slot number there when there is no queue), [5] step limit and [6] flags of that
 *       dialogue (queue only; bit 0: an eos does not end it), [7] reserved, 0 (cvx_t2s_decode_steps_mixed: the slot's role); x must hold start_token and state[0..2] zeros
 *       before a slot's first step.
 *   Continuous batching (queue != NULL; reference loop per dialogue: text2semantic.py:749-848, its exit :803-818): queue
 *       int32[2] = {next pending dialogue, number of dialogues}; dialogues int32[n][8]: the caller writes [0] context rows,
 *       [1] step limit (<= uniform_steps, <= max_len), [2] flags; the device writes [3] status (0 pending, 1 running, 2 ended
 *       by its eos, 3 by its limit), [4] steps decoded, [5] the slot it ran in.  A slot whose dialogue ends takes the next
 *       pending one inside the sampling kernel of the same step (position 0, `start` as input) or idles when none is left;
 *       the caller fills the first `batch` slots itself (slot b <- dialogue b, queue[0] = batch).
 *   Continuous batching under guidance (queue != NULL and cfg_scale > 1): a guided utterance u occupies the dialogue records 2u
 *       (text context; its uniforms and token row are the utterance's) and 2u + 1 (null context: [0] context rows = 1, kv_c row 0
 *       of that record = the learned null key / value); the caller writes [1] and [2] of both alike.  The queue still counts
 *       RECORDS: queue[1] = n_dialogues = twice the number of utterances (an odd n_dialogues is refused), and slot pair
 *       (2s, 2s + 1) starts on records (2s, 2s + 1) with queue[0] = batch.  The even slot decides when the pair ends (eos unless
 *       flag bit 0, or the step limit), writes [3] status, [4] steps and [5] slot into record 2u, MIRRORS them into record 2u + 1
 *       ([3] and [4] equal, [5] = the odd slot), takes the next two records from the queue and re-arms both slots (position 0,
 *       `start` as input of both); a pair is taken only if both of its records lie below queue[1]; with none left both slots
 *       idle.  The token row of record 2u + 1 is a copy of that of 2u, as in the lock-step guided decode.
 *   Filter (filter_mode): CVX_T2S_FILTER_TOP_K keeps the top_k largest logits (text2semantic.py:126-132: the reference's default is
 *       top_k = ceil(0.1 * vocab); an entry is kept iff fewer than top_k logits are larger, so entries equal to the top_k-th
 *       largest are all kept - torch.topk leaves open which of them it picks).  CVX_T2S_FILTER_TOP_P keeps entry i
 *       iff the softmax mass of the entries sorted before it is <= top_p (:118-124), where "sorted before" means a larger logit, or
 *       an equal logit at a lower index (the reference's torch.sort leaves the order of ties open).  Both act on the raw logits -
 *       the guidance-combined ones under cfg_scale > 1 - before the temperature division and the Gumbel noise, and the kept set
 *       is a function of the logits and the setting alone (not of the slot, the batch or the launch shape).
 *   Log-probabilities (cvx_t2s_decode_steps_scored only): every step also stores the log-probability the model gave the step's token,
 *       lp = (l[tok] - m) - logf(sum_j expf(l[j] - m)) with m = max_j l[j], into logprobs[(dialogue * streams + s) * max_len + pos] - a float
 *       buffer laid out like tokens.  l is the row the filter sees: the raw logits, or the guidance-combined ones under cfg_scale > 1 (then
 *       the value goes to record 2u; record 2u + 1 is unspecified) - before the filter, the temperature division and the Gumbel noise.  The
 *       sum runs in one fixed order (lane t of a wave adds the entries t, t + 64, ..., t + 960 in ascending order, entries past vocab being
 *       0, then the xor butterfly 32, 16, ..., 1 over the 64 lanes), so lp is a function of the row alone: not of the slot, the batch, the
 *       refills or the launch shape.
 *   Forced dialogues (cvx_t2s_decode_steps_scored only; cvx_t2s_decode_steps ignores the bit): flag bit 1 (value 2) of slot record [6] /
 *       dialogue record [2] - honoured in the slot record with and without a queue.  The token row of a forced dialogue already holds its
 *       tokens, each inside [0, vocab) (the caller checks; the device clamps a stray one): every step reads tokens[..., pos] instead of
 *       sampling, reads no uniforms of that record, stores the token's log-probability and feeds the token's embedding (to both slots of a
 *       guided pair).  An eos never ends a forced dialogue: only its step limit does (slot record [5] = the number of tokens to score), in
 *       a queue as for every dialogue (status 3); without a queue the slot then sets [1] = 1, [2] = the limit and idles at position max_len.
 *       Forced and sampled dialogues may share a queue; the log-probabilities of a sampled dialogue equal, bit for bit, those of the forced
 *       dialogue over the tokens it sampled.
 * The caller must not ask for more than max_len steps per slot without a queue (extra steps are ignored on the device).
 */
typedef struct {
    const float *gamma_s, *wqkv_s, *wo_s;        /* self-attention: norm.gamma, packed to_q|to_kv, to_out [dim, inner] */
    const float *gamma_c, *wq_c, *wo_c;          /* cross-attention */
    const float *kv_c;
    const float *gamma_f, *w1, *b1, *w2, *b2;    /* FeedForward: RMSNorm gamma, Linear(dim, 2F)+b, Linear(F, dim)+b */
    float *k_cache, *v_cache;                    /* [max_len, inner] */
} cvx_t2s_layer;

typedef struct {
    int32_t dim, inner, heads, ff_inner, ff_inner_pad, depth, streams, vocab, dim_emb, n_ctx, max_len, top_k;
    int32_t batch, ctx_rows;                     /* slots decoded together (1..64); kv_c rows allocated per dialogue */
    float temperature;
    const cvx_t2s_layer* layers;                 /* HOST array of `depth` entries */
    const float *final_gamma, *emb, *rope_cos, *rope_sin, *uniforms;
    float *x, *q, *att, *h, *logits;             /* per utterance: [dim], [inner], [inner], [ff_inner_pad], [streams, vocab] */
    int64_t* tokens;
    int32_t* state;
    float cfg_scale;                             /* <= 1: off.  > 1: classifier-free guidance (text2semantic.py:780-792), streams == 1, batch
                                                  * even: slot 2u decodes with the text context, slot 2u + 1 with the context masked out
                                                  * (state[3] = 1: the null key / value row only); every step samples slot 2u's token from
                                                  * null + (cond - null) * cfg_scale (uniforms of slot 2u) and feeds it to both slots */
    int32_t uniform_steps;                       /* steps of uniforms allocated per dialogue */
    int32_t* queue;                              /* NULL: slot b decodes dialogue b until the caller stops.  Else continuous batching (above) */
    int32_t* dialogues;
    const float* start;                          /* [dim] start token: the input of a slot that takes a new dialogue (queue != NULL) */
    int32_t filter_mode;                         /* CVX_T2S_FILTER_TOP_K (0; top_k must lie in [1, vocab]) or CVX_T2S_FILTER_TOP_P (top_k unused) */
    float top_p;                                 /* CVX_T2S_FILTER_TOP_P: the threshold, inside (0, 1) */
    int32_t n_dialogues;                         /* host copy of queue[1] (0: not given).  Required - positive and even - for a queue under
                                                  * guidance; the device still reads queue[1] */
} cvx_t2s_decoder;

#define CVX_T2S_FILTER_TOP_K 0
#define CVX_T2S_FILTER_TOP_P 1

/* CVX_EINVAL (nothing is launched) for an unknown filter_mode, top_k outside [1, vocab], top_p outside (0, 1) or an odd n_dialogues under
 * guidance, as for every other inconsistent descriptor. */
int cvx_t2s_decode_steps(const cvx_t2s_decoder* dec, int32_t n_steps, cvx_stream_t stream);

/* cvx_t2s_decode_steps with the log-probability epilogue and the forced mode (the comment block above): the same step chain, its sampling
 * kernel in the scoring instantiation.  struct_size = sizeof(cvx_t2s_scoring) - any other size is CVX_EINVAL; logprobs [dialogues, streams,
 * max_len] fp32 on the device (NULL is refused); logprob_len = floats per row of it, which must equal dec->max_len.  Every consistency check
 * of cvx_t2s_decode_steps applies; a refused call launches nothing. */
typedef struct {
    uint32_t struct_size;
    int32_t logprob_len;
    float* logprobs;
} cvx_t2s_scoring;

int cvx_t2s_decode_steps_scored(const cvx_t2s_decoder* dec, const cvx_t2s_scoring* scoring, int32_t n_steps, cvx_stream_t stream);

/* Per-dialogue sampling settings and forced prefixes: the step chain of cvx_t2s_decode_steps (scoring == NULL) or of
 * cvx_t2s_decode_steps_scored (scoring != NULL, checked as there), ending in a sampling kernel that takes its settings, per slot and per
 * step, from row `d` of a device-resident table - d being the DIALOGUE the slot decodes (slot record [4]), not the slot, so a slot that
 * the queue refills samples with the new dialogue's settings from its first step.
 *   table [n_records][8] 32-bit words, one row per dialogue record:
 *     [0] float inv_temp     1.0f / fmaxf(temperature, 1e-10f) computed in fp32 (the bits cvx_t2s_decode_steps computes from dec->temperature)
 *     [1] int32 filter_mode  CVX_T2S_FILTER_TOP_K or CVX_T2S_FILTER_TOP_P, chosen per step (block-uniform)
 *     [2] int32 top_k        [3] float top_p      the setting of that mode, as in cvx_t2s_decoder
 *     [4] float cfg_scale    read only in the guided pair layout: the even slot combines null + (cond - null) * cfg_scale with ITS dialogue's scale
 *     [5] int32 prefix_len   P >= 0, below        [6], [7] reserved, 0
 *   dec->temperature, filter_mode, top_k and top_p are ignored and need not be valid.  dec->cfg_scale keeps only its role as the layout
 *   switch: > 1 means slot pairs and record pairs (above), and row 2u + 1 of a pair mirrors row 2u (only row 2u is read).  With dec->queue
 *   and without (slot b then decodes dialogue b and reads row b).
 *   Prefix: while a slot's position is below P the step is a forced step (Forced dialogues, above) - it reads tokens[..., pos] of the
 *   dialogue's token row (clamped into [0, vocab)), reads no uniforms, feeds the token's embedding (to both slots of a guided pair), stores
 *   the token's log-probability when scoring != NULL, and an eos among these tokens does not end the dialogue.  From position P on the step
 *   samples as cvx_t2s_decode_steps does; uniforms stay indexed by position, so the rows below P are never read.  The forced read exists
 *   with and without scoring; flag bit 1 (a wholly forced dialogue) is honoured with scoring only, as in cvx_t2s_decode_steps_scored.
 *   Clamps: stray table values index nothing - the device clamps top_k into [1, vocab], takes an unknown mode as top-k, clamps P into
 *   [0, step limit] (slot record [5]; [0, max_len] without a queue) and a record number outside the table onto its first / last row.  The
 *   caller validates what it writes; the device does not report.
 *   Bit identity: every dialogue gets the tokens and log-probabilities it gets from cvx_t2s_decode_steps(_scored) alone with its row's
 *   settings in the descriptor - whatever the other rows hold, whichever slot it runs in; a dialogue with prefix P gets from position P on
 *   what the un-prefixed decode gets when it sampled the same P tokens.
 * No host synchronisation; graph-capturable.  CVX_EINVAL, nothing launched: struct_size != sizeof(cvx_t2s_per_dialogue), per or table NULL,
 * n_records < 1, n_records < dec->n_dialogues (when given) or, without a queue, < dec->batch, and everything cvx_t2s_decode_steps(_scored)
 * refuses apart from the ignored scalars. */
typedef struct cvx_t2s_per_dialogue {
    uint32_t struct_size;
    int32_t n_records;
    const void* table;
} cvx_t2s_per_dialogue;

int cvx_t2s_decode_steps_per_dialogue(const cvx_t2s_decoder* dec, const cvx_t2s_scoring* scoring, const cvx_t2s_per_dialogue* per,
                                      int32_t n_steps, cvx_stream_t stream);

/* Guided and unguided dialogues in ONE slot pool: the chain of cvx_t2s_decode_steps_per_dialogue (scoring NULL or not, the settings table
 * always) in which the pair layout is a property of the dialogue RECORD, not of the launch.  Still ABI 113: a symbol and a struct added.
 *   Dialogue records: flag bit 2 (CVX_T2S_FLAG_GUIDED, value 4) of record [2] makes record r the TEXT half of a guided utterance and
 *       record r + 1 its NULL half: [0] context rows = 1, kv_c row 0 of that record = the learned null key / value, [1], [2] and the
 *       settings row mirror those of record r.  An unguided utterance is one record.  queue[1] still counts records, and records may come
 *       in any mixture and order.  Uniforms, token row and log-probs of a guided utterance are those of record r; the token and log-prob
 *       rows of record r + 1 are unspecified (nothing in the chain reads them).
 *   Slot records: [7] is the slot's role - 0 a single slot, p + 1 the text half whose null half is slot p, -(p + 1) the null half of slot
 *       p.  Partners need not be neighbours.  dec->cfg_scale is not a layout switch here (> 1 is refused); the scale of a guided utterance
 *       is word [4] of its settings row.
 *   Sampling (one block per slot): an idle slot and a null half return at once; a single slot samples as the per-dialogue chain does
 *       without guidance; a text half as it does under guidance, from null + (cond - null) * scale with the null half's logits row, and
 *       feeds the token's embedding to both slots.  Prefixes, forced dialogues and log-probs as in cvx_t2s_decode_steps_per_dialogue.
 *       A dialogue that ends (eos unless flag bit 0, or its step limit) gets [4] steps, [5] slot and then [3] status written into its
 *       record - and into the null record of a pair, with [5] = the null half's slot - and its slot(s) idle: [0] = max_len, [1] = 1,
 *       [7] = 0 (the null half's [7] is cleared by the scheduler launch that follows: its own block may still be reading it).  The
 *       sampling launch does not touch the queue.
 *   Scheduler (one block, one launch after the sampling launch of every step; the kernel boundary orders it behind every record write):
 *       F = the idle slots ([0] >= max_len) in ascending order.  Loop: h = queue[0]; stop if h >= queue[1] or F is empty.  Record h
 *       unguided: the lowest slot of F takes it, h += 1.  Guided: stop if h + 1 >= queue[1] (a pair is taken only if both records exist)
 *       or F holds fewer than two slots (the head WAITS - strict queue order, no look-ahead); else the lowest slot of F becomes the text
 *       half of record h, the next one the null half of record h + 1, h += 2.  A slot that takes a record starts at position 0 with
 *       `start` as its input, [3]..[6] from the record, its role in [7]; the record gets [3] = 1 and [5] = the slot.  Serial and
 *       deterministic: which slots an utterance runs in is a function of the records and of the step every utterance ends at.
 *   n_steps == 0 runs the scheduler once and nothing else: with every slot idle ([0] = max_len) and queue = {0, n} that ARMS a call, so
 *       the policy exists in one place.
 *   mixed->n_guided: the number of guided utterances among the records (the host's count; the device reads the flags).
 *   Bit identity: every utterance, guided or not, gets the tokens and log-probs it gets alone from cvx_t2s_decode_steps(_scored) with its
 *   settings - whichever slots it runs in, whatever its neighbours are.
 * No host synchronisation; graph-capturable; per step the launches of cvx_t2s_decode_steps plus one.  CVX_EINVAL, nothing launched:
 * struct_size != sizeof(cvx_t2s_mixed), mixed, per or dec->queue NULL, dec->cfg_scale > 1, n_guided < 0 or 2 * n_guided >
 * dec->n_dialogues, n_guided > 0 with streams != 1 or batch < 2, and everything cvx_t2s_decode_steps_per_dialogue refuses. */
#define CVX_T2S_FLAG_GUIDED 4

typedef struct cvx_t2s_mixed {
    uint32_t struct_size;
    int32_t n_guided;
} cvx_t2s_mixed;

int cvx_t2s_decode_steps_mixed(const cvx_t2s_decoder* dec, const cvx_t2s_scoring* scoring, const cvx_t2s_per_dialogue* per,
                               const cvx_t2s_mixed* mixed, int32_t n_steps, cvx_stream_t stream);

/* History rules: the chain of cvx_t2s_decode_steps_per_dialogue (mixed == NULL) or of cvx_t2s_decode_steps_mixed (mixed != NULL), ending
 * in sampling kernels that first change the row the filter sees by what the stream has ALREADY EMITTED.  Still ABI 113: symbols and a struct
 * added; cvx_t2s_per_dialogue, its 8-word rows and every other entry point are untouched.
 *   rules->table [n_records][4] 32-bit words, one row per dialogue record, indexed like the settings table (a null half mirrors its text half):
 *     [0] float theta   repetition penalty, > 0; 1 is off        [1] int32 window W >= 0; 0 = the whole history
 *     [2] int32 ngram   n in 0..8; 0 is off                      [3] int32 min_len m >= 0
 *   Per output stream s of a dialogue at position pos, h = tokens[dialogue][s][0, pos) - the stream's own token row, a forced prefix
 *   included; a refilled slot names a new dialogue and so starts with an empty history.  On the row the filter would see (the
 *   guidance-combined row for a pair), in this order, before the filter, the temperature and the noise:
 *     1. every id that occurs in h[max(0, pos - W), pos) is penalised ONCE: l = l > 0 ? l / theta : l * theta (an IEEE fp32 division);
 *     2. for every j in [0, pos - n] with h[j, j + n - 1) == h[pos - n + 1, pos) the id h[j + n - 1] becomes -inf (n = 1: every id of h);
 *     3. while pos < m the eos (vocab - 1) becomes -inf.
 *   If no entry is finite after 3, the bans of 2 are void for this step; 1 and 3 stay.  The eos is an id like any other for 1 and 2.
 *   Given steps (a prefix, a forced dialogue) select nothing: the rules do not act there.  Log-probabilities stay the model's: with
 *   scoring they are the log-softmax of the row BEFORE the rules, so they equal, bit for bit, the teacher-forced log-probs of the same tokens.
 *   A neutral row (theta = 1, n = 0, m = 0) gives the tokens and log-probs of the chain without rules, bit for bit.
 *   Clamps: the device takes n into [0, 8], W and m into [0, max_len], theta <= 0 or NaN as 1, a record number outside the table onto its
 *   first / last row, and an id outside [0, vocab) in the history marks nothing.
 * No host synchronisation; graph-capturable; the launches of the chain it stands for.  CVX_EINVAL, nothing launched: struct_size !=
 * sizeof(cvx_t2s_rules), rules or table NULL, n_records < 1 or below what `per` must hold (dec->n_dialogues; without a queue dec->batch),
 * and everything cvx_t2s_decode_steps_per_dialogue (mixed == NULL) or cvx_t2s_decode_steps_mixed refuses. */
typedef struct cvx_t2s_rules {
    uint32_t struct_size;
    int32_t n_records;
    const void* table;
} cvx_t2s_rules;

int cvx_t2s_decode_steps_rules(const cvx_t2s_decoder* dec, const cvx_t2s_scoring* scoring, const cvx_t2s_per_dialogue* per,
                               const cvx_t2s_mixed* mixed, const cvx_t2s_rules* rules, int32_t n_steps, cvx_stream_t stream);

/* The history rules alone, through the device code of the decode: out[r] = the row the filter would see for logits[r] [V <= 1024] after
 * the rules of table[r] (4 words, above; W and m only clamped at 0), with h = history[r][0, hist_len[r]) (int64 [rows, hist_ld]; hist_len
 * clamped into [0, hist_ld]; history may be NULL when hist_ld == 0) and pos = hist_len[r].  The inputs are not written.  CVX_EINVAL: a NULL
 * pointer, rows < 0, V outside [1, 1024], hist_ld < 0. */
int cvx_t2s_rules_f32(const float* logits, const int64_t* history, const int32_t* hist_len, const void* table, int64_t rows, int32_t V,
                      int32_t hist_ld, int32_t eos_id, float* out, cvx_stream_t stream);

/* Beam search on the decode slots - the deterministic decode behind the reference's beam_search_decode flag, which its generate accepts
 * and never implements (text2semantic.py:673-677): the algorithm below is this library's definition.
 * Per utterance: B = beam_size hypotheses (1 <= B <= 16) in B neighbouring slots; utterance u owns slots [u B, (u + 1) B), and
 * dec->batch = utterances * B <= 64.  S = streams, V = vocab, eos = V - 1.  One step:
 *   lp[s][j] = log_softmax of stream s's raw logits row exactly as defined under "Log-probabilities" above (same m, expf and summation tree);
 *       temperature, filter and uniforms play no part.
 *   Shortlist: per live hypothesis and stream the min(B, V) entries with the largest lp, ordered by (lp descending, index ascending): the
 *       rank of entry i is the number of entries j with lp[j] > lp[i], or lp[j] == lp[i] and j < i.
 *   Candidates of a live hypothesis p with cumulative score c[p]: S = 1: (p, a) scored c[p] + lp[0][tok_a]; S = 2: (p, a, b) scored
 *       c[p] + (lp[0][tok_a] + lp[1][tok_b]) - fp32 in this association; order key q = (p B + a) B + b (b = 0 for S = 1).  A FINISHED
 *       hypothesis (one that took an eos in any stream) has one candidate: itself, score unchanged, q = p B B.  A hypothesis with score
 *       -inf has none (before step 0 the caller gives hypothesis 0 score 0 and the others -inf).
 *   Selection: the B candidates with the largest score, ties to the lowest q; new slot i receives the i-th best.  A slot for which no
 *       candidate is left becomes a dead hypothesis: parent i, tokens -1, score -inf, finished.
 *   The utterance ends when all B hypotheses are finished, or at its step limit; its slots then idle at position max_len.
 * KV caches are never copied: a cache row (slot, position) is written once per utterance, by the hypothesis that sits in that slot at that
 * step, and owner int32 [2][batch][max_len] (ping-ponged by step parity; row ((pos & 1) * batch + slot)) names, for every past position of
 * the hypothesis in a slot, the slot whose cache holds it.  The self-attention of the beam chain reads key / value j from slot owner[..][j]
 * with the arithmetic, loop shape and accumulation order of the direct kernel (an identity table gives the same bits); the selection writes
 * the next row: the parent's row for positions 0..pos, then the slot itself.  The caller fills the table with the identity
 * (owner[*][slot][*] = slot) before step 0.  History is kept as back-pointers: parents [max_len][batch] (index INSIDE the group),
 * hist_tokens int32 / hist_logprobs fp32 [max_len][batch][streams] (a carried finished hypothesis records tokens -1, log-probs 0).
 * groups int32 [batch / B][4]: [0] steps done (the caller writes 0), [1] ended (the caller writes 0; 1 for a group that must stay idle),
 * [2] step limit (<= max_len), [3] reserved.  Slot records: the caller writes [0] = 0, [1] = 0, [2] = 0, [3] context rows and [4] the
 * dialogue (the B slots of an utterance name the same one) as for cvx_t2s_decode_steps (idle groups: [0] = max_len); the selection writes
 * [0] position (max_len once the hypothesis is finished or the utterance has ended), [1] finished-or-ended, [2] the steps the hypothesis
 * took up to and including its eos step (all steps when it never finished).  scores fp32 [batch] / finished uint8 [batch]: in and out.
 * short_lp fp32 / short_tokens int32 [batch][streams][16]: workspace.  backtrack != 0: after the n_steps steps (n_steps may be 0) a
 * back-track kernel writes dec->tokens int64 [batch][streams][max_len] and logprobs fp32 [batch][streams][max_len] (hist_len = max_len)
 * of the hypothesis in every slot from the back-pointers.  Per step: the launches of cvx_t2s_decode_steps plus one.  No host
 * synchronisation, graph-capturable.  CVX_EINVAL (nothing is launched): struct_size != sizeof, dec->queue != NULL, dec->cfg_scale > 1,
 * beam_size outside [1, 16], batch % beam_size != 0, hist_len != max_len, a NULL pointer, and everything cvx_t2s_decode_steps refuses. */
typedef struct cvx_t2s_beam {
    uint32_t struct_size;
    int32_t beam_size;
    int32_t hist_len;
    int32_t backtrack;
    float* scores;
    uint8_t* finished;
    int32_t* owner;
    int32_t* groups;
    int32_t* parents;
    int32_t* hist_tokens;
    float* hist_logprobs;
    float* short_lp;
    int32_t* short_tokens;
    float* logprobs;
} cvx_t2s_beam;

int cvx_t2s_beam_steps(const cvx_t2s_decoder* dec, const cvx_t2s_beam* beam, int32_t n_steps, cvx_stream_t stream);

/* Beam search through CONTINUOUSLY REFILLED slot groups: a list of n utterances runs through the dec->batch / B groups of B neighbouring
 * slots; a group whose utterance ends takes the next pending one inside the selection launch of that very step (no host round trip), as a
 * slot of the sampled decode takes the next dialogue.  The step chain, the selection and every hypothesis are those of cvx_t2s_beam_steps:
 * an utterance gets, bit for bit, what it gets alone.  dec->queue stays NULL (the dialogue queue of the sampled decode plays no part).
 *   beam: a complete cvx_t2s_beam as for cvx_t2s_beam_steps, with groups record [3] = the utterance the group decodes; its parents,
 *       hist_tokens, hist_logprobs and logprobs are not written (history is kept per utterance, below).
 *   queue int32[2] = {next pending utterance, number of utterances}; utterances int32[n][8]: the caller writes [0] context rows, [1] step
 *       limit; the device writes [3] status (0 pending, 1 running, 2 all hypotheses finished, 3 step limit), [4] steps decoded, [5] the group
 *       it ran in.  Slot record [4] of the B slots of a group names the utterance: it indexes kv_c as a dialogue does.  The caller starts group
 *       g on utterance g (g < min(groups, n)): slot and group records as for cvx_t2s_beam_steps, utterance records [3] = 1, [5] = g, and
 *       queue[0] = min(groups, n); groups beyond stay ended ([1] = 1, slots at max_len).  owner[0][slot][0] = slot for the slots that
 *       start; nothing else of the ancestry table needs a value.
 *   When a group's utterance ends - all B hypotheses finished, or t + 1 has reached its limit (clamped into [1, max_len]) - the selection
 *       launch writes final_scores fp32 / final_steps int32 / final_finished uint8 [n][B] (what scores, slot record [2] and finished hold
 *       at the end of cvx_t2s_beam_steps), status and steps, takes the next utterance with one atomicAdd on queue[0] (taken only below
 *       queue[1]) and re-arms the group: group record {0, 0, limit, utterance}, scores {0, -inf, ...}, finished 0, slot records position 0,
 *       [1] = [2] = 0, [3] = context rows (clamped into [1, ctx_rows]), [4] = utterance, x of all B slots = `start` ([dim] start token) and
 *       owner[0][slot][0] = slot.  With no utterance left the group ends, its slots idle at max_len.  Cache and ancestry rows of the ended
 *       utterance stay in place and are never read: the new utterance's ancestry rows name only positions it has written.
 *   History by UTTERANCE: parents int32 [n][hist_len][B], hist_tokens int32 / hist_logprobs fp32 [n][hist_len][B][streams].  backtrack != 0
 *       (in `beam`): after the n_steps steps (n_steps may be 0) one thread per (utterance, hypothesis) writes tokens int64 / logprobs fp32
 *       [n * B][streams][max_len] from the back-pointers over the steps utterance record [4] holds (the caller zeroes it).
 * No host synchronisation, graph-capturable (n_utterances sizes the back-track launch only; the steps read queue[1]).  CVX_EINVAL (nothing is
 * launched): struct_size != sizeof of either struct, a NULL pointer, n_utterances < 1, dec->queue != NULL, dec->cfg_scale > 1, beam_size
 * outside [1, 16], batch % beam_size != 0, hist_len != max_len, and everything cvx_t2s_decode_steps refuses. */
typedef struct cvx_t2s_beam_queue {
    uint32_t struct_size;
    int32_t n_utterances;
    int32_t* queue;
    int32_t* utterances;
    const float* start;
    int32_t* parents;
    int32_t* hist_tokens;
    float* hist_logprobs;
    float* final_scores;
    int32_t* final_steps;
    uint8_t* final_finished;
    int64_t* tokens;
    float* logprobs;
} cvx_t2s_beam_queue;

int cvx_t2s_beam_queue_steps(const cvx_t2s_decoder* dec, const cvx_t2s_beam* beam, const cvx_t2s_beam_queue* bq, int32_t n_steps,
                             cvx_stream_t stream);

/* Beam search UNDER CLASSIFIER-FREE GUIDANCE (dec->cfg_scale > 1, one-output models: streams == 1): the algorithm of cvx_t2s_beam_steps
 * with S = 1, where a hypothesis is a SLOT PAIR with one ancestry, as a guided utterance of the sampled decode is a slot pair.
 *   Layout: hypothesis h of the launch sits in slots 2h (the TEXT half: decodes with the text context) and 2h + 1 (the NULL half: decodes
 *       with the learned null key / value only).  Utterance u owns hypotheses [u B, (u + 1) B) = slots [2 u B, 2 (u + 1) B);
 *       dec->batch = utterances * 2 B <= 64, 1 <= B <= 16.  H = dec->batch / 2 hypotheses, G = H / B groups.
 *   Indexed BY SLOT (dec->batch rows, as in cvx_t2s_beam_steps): the slot records dec->state, owner int32 [2][batch][max_len], dec->x,
 *       dec->logits and the self-attention caches.
 *   Indexed BY HYPOTHESIS (H rows where cvx_t2s_beam_steps has batch rows): scores fp32 [H], finished uint8 [H], parents int32 [max_len][H]
 *       (index inside the group), hist_tokens int32 / hist_logprobs fp32 [max_len][H][1], short_lp fp32 / short_tokens int32 [H][1][16],
 *       the back-tracked dec->tokens int64 [H][1][max_len] and logprobs fp32 [H][1][max_len]; groups int32 [G][4] as before.
 *   The caller writes, before step 0: both slot records of hypothesis h of utterance u - text half {0, 0, 0, context rows of u, kv_c row of
 *       u's [null | context] block, ...}, null half {0, 0, 0, 1, a kv_c row whose row 0 holds the learned null key / value, ...} (the rows a
 *       guided pair of cvx_t2s_decode_steps uses; the B hypotheses of an utterance may share both); x of both slots = the start token; the
 *       identity ancestry owner[*][slot][*] = slot; scores {0, -inf, ...} per utterance, finished 0, groups {0, 0, limit, 0}.  Idle groups:
 *       groups [1] = 1 and both slots of every hypothesis at position max_len.
 *   One step: g[j] = n[j] + (c[j] - n[j]) * scale in fp32 in this operation order (no contraction), c = the logits row of the text half, n
 *       that of the null half, scale = dec->cfg_scale; lp[j] = log_softmax of g exactly as defined under "Log-probabilities" above - the
 *       row and the function the scored decode uses under guidance, so lp carries the bits cvx_t2s_decode_steps_scored gives a forced
 *       dialogue pair with the same prefix.  Shortlist, candidates, order key q, selection, ties, dead and finished hypotheses, the end of
 *       an utterance: cvx_t2s_beam_steps with S = 1, over hypotheses.
 *   The selection writes, for BOTH halves of new hypothesis i with parent p: the slot records ([0] position, or max_len for a finished
 *       hypothesis and for an ended utterance - both slots idle together; [1], [2] as in cvx_t2s_beam_steps); the next input - the chosen
 *       token's embedding row into both x rows; and the next ancestry rows - the text slot's row is the parent's TEXT row for positions
 *       0..pos, then the text slot itself; the null slot's row is the parent's NULL row, then the null slot itself.  The self-attention
 *       kernel is the one of cvx_t2s_beam_steps, one block row per slot.
 *   Per step: the launches of cvx_t2s_beam_steps, no more.  No host synchronisation, graph-capturable.  backtrack as in cvx_t2s_beam_steps,
 *       one thread per hypothesis.
 * CVX_EINVAL (nothing is launched): dec->cfg_scale not > 1 (NaN included; cvx_t2s_beam_steps is the unguided entry), streams != 1,
 * n_ctx != 0, dec->queue != NULL, beam_size outside [1, 16], batch % (2 beam_size) != 0, hist_len != max_len, struct_size != sizeof, a
 * NULL pointer, and everything cvx_t2s_decode_steps refuses. */
int cvx_t2s_beam_guided_steps(const cvx_t2s_decoder* dec, const cvx_t2s_beam* beam, int32_t n_steps, cvx_stream_t stream);

/* cvx_t2s_beam_queue_steps under guidance: the G = dec->batch / (2 B) groups of cvx_t2s_beam_guided_steps, refilled from a list of n
 * utterances.  `beam` as for cvx_t2s_beam_guided_steps (groups record [3] = the utterance), `bq` as for cvx_t2s_beam_queue_steps: its
 * arrays are by utterance and hypothesis already ([n][hist_len][B]..., [n][B], [n * B][1][max_len]).  Utterance j owns TWO kv_c rows, as a
 * guided record pair of the sampled decode does: row 2 j holds [null | context of j] (utterance record [0] = its context rows), row 2 j + 1
 * holds the learned null key / value in its row 0.  The caller starts group g on utterance g: text slots {0, 0, 0, context rows, 2 g, ...},
 * null slots {0, 0, 0, 1, 2 g + 1, ...}, owner[0][slot][0] = slot for both halves.  A refilled group re-arms BOTH halves of its B
 * hypotheses: x = start, position 0, [1] = [2] = 0, owner[0][slot][0] = slot, text half [3] = context rows (clamped into [1, ctx_rows]) and
 * [4] = 2 * utterance, null half [3] = 1 and [4] = 2 * utterance + 1.  Everything else, the finals and the back-track included, is
 * cvx_t2s_beam_queue_steps; an utterance gets, bit for bit, what cvx_t2s_beam_guided_steps gives it alone.  CVX_EINVAL: what
 * cvx_t2s_beam_guided_steps and cvx_t2s_beam_queue_steps refuse (with cfg_scale not > 1 refused here, cfg_scale > 1 there). */
int cvx_t2s_beam_guided_queue_steps(const cvx_t2s_decoder* dec, const cvx_t2s_beam* beam, const cvx_t2s_beam_queue* bq, int32_t n_steps,
                                    cvx_stream_t stream);

/* The selection step alone (the device functions cvx_t2s_beam_steps selects with; no slot state): groups G of beam_size B hypotheses,
 * logits [G * B, streams, V] fp32, scores_in [G * B], finished_in uint8 [G * B] -> per new slot: parents (index inside the group), tokens
 * int64 [G * B, streams] and token_lp fp32 [G * B, streams] (-1 and 0 for a carried or dead hypothesis), scores_out, finished_out.  Groups
 * do not influence each other.  CVX_EINVAL (nothing is launched) for beam_size outside [1, 16], streams outside {1, 2}, V outside
 * [1, 1024], groups < 0 or a NULL pointer. */
int cvx_t2s_beam_select_f32(const float* logits, const float* scores_in, const uint8_t* finished_in, int32_t groups, int32_t beam_size,
                            int32_t streams, int32_t V, int32_t* parents, int64_t* tokens, float* token_lp, float* scores_out,
                            uint8_t* finished_out, cvx_stream_t stream);

/* Beam search UNDER THE HISTORY RULES no-repeat n-gram and minimum length: cvx_t2s_beam_steps (bq == NULL, dec->cfg_scale <= 1),
 * cvx_t2s_beam_guided_steps (bq == NULL, dec->cfg_scale > 1), cvx_t2s_beam_queue_steps or cvx_t2s_beam_guided_queue_steps (bq != NULL, by
 * dec->cfg_scale) - their structs, layouts, launches and results - with shortlist and merge kernels that first REMOVE candidates.  Still ABI
 * 113: two symbols added, no struct changed.  A hypothesis' score stays the sum of the model's log-probabilities: nothing is renormalised,
 * nothing is penalised.
 *   1. History.  For a live hypothesis at position pos and output stream s, h_s holds the pos tokens its ANCESTRY took in stream s, oldest
 *      first.  A live hypothesis has taken no eos, so h_s holds ids in [0, V - 1) only.  A re-armed group (queue forms) starts a new
 *      utterance with an empty history.  The device reads it along the ancestry table: owner[pos & 1][slot][j + 1] names the slot the
 *      ancestor sat in after step j, whose hist_tokens entry of step j is h_s[j] (the text half's row and slot / 2 in the guided chain).
 *   2. Order.  lp[s][j] is computed exactly as in cvx_t2s_beam_steps / cvx_t2s_beam_guided_steps: the log_softmax of the raw row, or of the
 *      guidance-combined row, the same function and the same bits.  The bans are applied AFTER it, as -inf on lp.
 *   3. The two bans.  No-repeat n-gram, n in 1..8: for every j in [0, pos - n] with h_s[j, j + n - 1) == h_s[pos - n + 1, pos) the id
 *      h_s[j + n - 1] is banned (n = 1: every id of h_s) - point 2 of cvx_t2s_rules, word for word.  Minimum length m: while pos < m the eos
 *      (V - 1) is banned in every stream.
 *   4. Void bans.  If the bans leave no un-banned entry in stream s's row, the n-gram bans of that stream are void for this step and the eos
 *      ban stays (as in the sampled chain).
 *   5. Shortlist and merge.  The shortlist ranks the banned lp with the order of cvx_t2s_beam_steps (lp descending, index ascending).  A
 *      shortlist entry whose lp is -inf gives no candidate; a live hypothesis with no candidate left contributes none; a new slot for which
 *      no candidate is left becomes a dead hypothesis exactly as cvx_t2s_beam_steps defines it.
 *   6. What stays the model's.  hist_logprobs, the back-tracked logprobs, scores and final_scores are the model's log-probs and their fp32
 *      sums in the association of cvx_t2s_beam_steps: every returned hypothesis' log-probs equal, bit for bit, the teacher-forced log-probs
 *      of its tokens (under dec->cfg_scale in the guided chain), and its score is the fp32 sum the selection kept.
 *   7. The table.  rules->table [n_records][4] words as in cvx_t2s_rules, one row per UTTERANCE: row = group index in the lock-step forms,
 *      row = utterance number (groups record [3]) in the queue forms.  The device reads [2] (n, clamped into [0, 8]) and [3] (m, clamped into
 *      [0, max_len]) and ignores [0] and [1]: beam search has no repetition penalty (it would make the search score something other than the
 *      model's log-probability).  A row with n = 0 and m = 0 gives the chain without rules, bit for bit.
 * Per step: the launches of the chain it stands for, no more.  No host synchronisation, graph-capturable.  CVX_EINVAL, nothing launched:
 * rules->struct_size != sizeof(cvx_t2s_rules), rules or table NULL, n_records below the groups of the launch (lock-step: dec->batch /
 * beam_size, or / (2 beam_size) guided) or below bq->n_utterances (queue), and everything the entry point of the same form refuses. */
int cvx_t2s_beam_rules_steps(const cvx_t2s_decoder* dec, const cvx_t2s_beam* beam, const cvx_t2s_beam_queue* bq /* NULL: lock-step */,
                             const cvx_t2s_rules* rules, int32_t n_steps, cvx_stream_t stream);

/* cvx_t2s_beam_select_f32 under those rules, through the device code of cvx_t2s_beam_rules_steps: the history is given outright - history
 * int32 [G * B][streams][hist_ld] (may be NULL when hist_ld == 0), hist_len int32 [G * B] (= pos of the hypothesis, clamped into
 * [0, hist_ld]) - and table holds one 4-word row per GROUP ([2] n, clamped into [0, 8]; [3] m, clamped at 0 only: there is no max_len
 * here).  Same outputs.  CVX_EINVAL (nothing is launched): what cvx_t2s_beam_select_f32 refuses, hist_ld outside [0, 4096]. */
int cvx_t2s_beam_select_rules_f32(const float* logits, const float* scores_in, const uint8_t* finished_in, const int32_t* history,
                                  const int32_t* hist_len, const void* table, int32_t groups, int32_t beam_size, int32_t streams, int32_t V,
                                  int32_t hist_ld, int32_t* parents, int64_t* tokens, float* token_lp, float* scores_out,
                                  uint8_t* finished_out, cvx_stream_t stream);

/* The log-probability epilogue alone (the device function cvx_t2s_decode_steps_scored uses): out[r] = log_softmax(logits[r, :])[tokens[r]]
 * as defined above; logits [rows, V] fp32, tokens int64 [rows], out fp32 [rows].  One thread block per row.  A token outside [0, V) gives
 * its row a NaN.  CVX_EINVAL (nothing is launched) for V < 1, V > 1024, rows < 0 or a NULL pointer. */
int cvx_t2s_logprob_f32(const float* logits, const int64_t* tokens, int64_t rows, int32_t V, float* out, cvx_stream_t stream);

/* PREFILL: the attention of one causal full-sequence pass of the target transformer over tokens that are already known (a forced
 * dialogue, a forced prefix) - csrc/t2s_prefill.hip.  Still ABI 113: symbols and a struct added.
 * The pass (neurips2024-covomix_amd/t2s.py, _prefill): a packed batch of n sequences; sequence i has L_i input rows at positions
 * 0 .. L_i - 1 (row 0 = start_token, row p > 0 = the embeddings of its tokens at p - 1, stream after stream) and runs the decoder
 * layers in the order of cvx_t2s_decode_steps on all rows at once: the row-local parts on the full-sequence kernels (fp32 GEMM with the
 * half-split RoPE epilogue at the row's position, RMSNorm, GEGLU), the two attentions through this entry.  Logits row p is the pre-filter
 * row of decode step p; the rows are fp32-class, not bit-identical to the step chain (a GEMM and a GEMV round differently).
 * One call, both modes.  Query row r of sequence i (cu[i] <= r < cu[i + 1]), at index p = r - cu[i], head h:
 *     out[r][h] = softmax_j(scale * q[r][h] . K[kbase[i] + j][h]) . V[kbase[i] + j][h]     over j < (causal ? p + 1 : nk[i])
 *   q   [rows][ldq], k / v [*][ldkv] (one shared row stride), out [rows][heads * 64], all fp32, heads of 64 columns side by side;
 *   cu int32 [n + 1] (cu[0] = 0, cu[n] = rows), kbase int32 [n] (first key row of sequence i), nk int32 [n] (its key count, >= 1;
 *   not read - may be NULL - when causal), all on the device; max_q = the largest cu[i + 1] - cu[i] (the host's copy: it sizes the grid).
 *   Self-attention of the pass: the packed q | k | v buffer itself - k = qkv + inner, v = qkv + 2 inner, ldq = ldkv = 3 inner,
 *   kbase = cu, causal = 1.  Cross-attention: the decode's kv_c records directly - v = k + inner, ldkv = 2 inner,
 *   kbase[i] = record * ctx_rows, nk[i] = context rows (row 0 is the null key / value), causal = 0; no RoPE, no mask but the count.
 * Flash-style online softmax in the exp2 domain; nothing rows x keys reaches memory.  A key is SELECTED by its index, not masked by
 * adding a large number: key rows at or past a sequence's count (causal: past its last row) are never read and may hold anything, NaN
 * included.  (Causal: the rows of the sequence itself that lie behind a query's position share its tiles - their scores are not
 * selected, their weights are exactly 0, and their v must be finite, as rows of one pass are.)  A block works on one sequence only, and
 * a query's result does not depend on the other sequences of the call nor - causal - on any row behind its position.  No scratch.
 * CVX_EINVAL, nothing launched: p NULL, struct_size != sizeof(cvx_t2s_prefill_attention), n < 1, heads < 1, rows < 0, max_q outside
 * [0, rows]; with rows > 0: a NULL pointer (nk only when not causal), max_q < 1, a stride below heads * 64 or not a multiple of 4, a
 * pointer off 16 bytes.  rows == 0 is a no-op returning 0. */
typedef struct cvx_t2s_prefill_attention {
    uint32_t struct_size;
    int32_t n, heads, causal, max_q;
    float scale;
    int64_t rows;
    const float* q;
    int64_t ldq;
    const float *k, *v;
    int64_t ldkv;
    float* out;
    const int32_t *cu, *kbase, *nk;
} cvx_t2s_prefill_attention;

int cvx_t2s_prefill_attention_f32(const cvx_t2s_prefill_attention* p, cvx_stream_t stream);

/* Guidance on the logits rows of a pass: for r < rows with null_row[r] >= 0,  l[r][c] = n + (l[r][c] - n) * scale[r]  with
 * n = l[null_row[r]][c] - the operation order of the guided decode step, no contraction; a row with null_row[r] < 0 is left alone.
 * logits fp32 [>= rows][width] (the null rows lie behind `rows` and are only read), null_row int32 [rows], scale fp32 [rows], on the
 * device.  CVX_EINVAL (nothing is launched): a NULL pointer, rows < 0, width < 1. */
int cvx_t2s_prefill_guidance_f32(float* logits, const int32_t* null_row, const float* scale, int64_t rows, int32_t width,
                                 cvx_stream_t stream);

/* EDIT DISTANCE of many pairs of token sequences in one launch - csrc/edit_distance.hip.  Still ABI 113: one symbol and one constant added.
 * What consensus (minimum-Bayes-risk) selection among the candidates of best-of-N and the reference's validation metric of
 * text2semantic (covomix/util/inference.py:287-358: jiwer.wer over token strings) are counted with.
 *   out[p] = the unit-cost Levenshtein distance between items a_p and b_p: the fewest substitutions, insertions and deletions (1 each)
 *            that turn one into the other.
 * tokens int64 [n_tokens] on the device; an ITEM is tokens[offset : offset + length), 0 <= length <= CVX_EDIT_MAX_LEN; items may overlap,
 * touch or repeat.  items = int32 [n_items][2] (offset, length), pairs = int32 [n_pairs][2] (item a, item b), each given twice: the
 * HOST copy is validated before anything is launched and sizes the launch, the DEVICE copy is what the kernel reads (the caller uploads
 * it; nothing is copied or allocated here, no host synchronisation, graph-capturable).  out int32 [n_pairs] on the device.
 * Tokens are compared by their low 32 bits (the kernel narrows them; every vocabulary here is far below 2^31).  A zero-length item gives
 * the other item's length; a pair may name one item twice (0) and pairs may repeat; a pair's result depends on its two items alone, not
 * on its place in the table or on its neighbours.  One block per pair, ONE store per pair, int32 arithmetic, no global scratch, no
 * atomics, no token behind an item's length read.
 * CVX_EINVAL, nothing launched and out untouched: a negative count; an item with offset < 0, length outside [0, CVX_EDIT_MAX_LEN] or
 * offset + length > n_tokens; a pair index outside [0, n_items); a NULL table; with n_pairs > 0 a NULL device pointer.  n_pairs == 0 is
 * a successful call without a launch.  A block whose DEVICE rows break these bounds (the device copy is not the host copy) reads no
 * token and stores -1. */
#define CVX_EDIT_MAX_LEN 4096           /* tokens per item: two streams of the largest max_length */
int cvx_edit_distance_i64(const int64_t* tokens_dev, int64_t n_tokens, const int32_t* items_host, const int32_t* items_dev, int32_t n_items,
                          const int32_t* pairs_host, const int32_t* pairs_dev, int32_t n_pairs, int32_t* out_dev, cvx_stream_t s);

/* DTW: dynamic time warping of many pairs of feature sequences in one launch - csrc/dtw.hip.
 * Still ABI 113: one symbol and two constants added.  What the mel-cepstral distortion of the acoustic model's output against a target of another timing is counted with
 * (metrics.py; the reference validates the acoustic model by a frame-wise F.mse_loss, covomix/util/inference.py:32-75, :151-227, which
 * needs equal timing).
 *   cost_dev[p], steps_dev[p] = the cost and the length (cells) of the best warping path between items a_p and b_p.
 * frames fp32 [n_rows][ld] on the device; an ITEM is rows [first row, first row + frames), 0 <= frames <= CVX_DTW_MAX_FRAMES; items may
 * overlap or repeat.  1 <= dim <= CVX_DTW_MAX_DIM, ld >= dim, ld % 4 == 0, frames_dev 16-byte aligned.  Columns [dim, ld) and rows outside
 * every item may hold anything (NaN included): they are not read into a result.  items = int32 [n_items][2] (first row, frames), pairs =
 * int32 [n_pairs][2] (item a, item b), each given twice as for cvx_edit_distance_i64: the HOST copy is validated before anything is
 * launched and sizes the launch, the DEVICE copy is what the kernel reads; nothing is copied or allocated here, no host
 * synchronisation, graph-capturable.
 * The definition, fixed to the bit:
 *   frame distance  c(i, j) = sqrt(sum_d (x_i[d] - y_j[d])^2), d ascending, the sum starting from +0, every subtraction, product, sum and
 *                   the square root an individually rounded fp32 operation (no contraction).  Dimensions an instance pads behind dim
 *                   add (0 - 0)^2 = +0, which changes no bit.
 *   path            steps (i-1, j-1), (i-1, j), (i, j-1), unit weights, no window.  A cell carries (cost, steps):
 *                   cost(i, j) = c(i, j) + the smallest cost among its predecessors (one rounded fp32 sum), steps(i, j) = 1 + the
 *                   SMALLEST steps among the predecessors of that cost - a lexicographic minimum on (cost, steps).  Cell (0, 0) is
 *                   (c(0, 0), 1).  The rule is symmetric: a pair and its swap give the same bits.
 *   result          the last cell; (0.0f, 0) if either item has no frame.  Non-finite features leave that pair's result unspecified
 *                   (no other pair's, and nothing is read out of bounds).
 * A pair's result depends on its two items alone: not on its place in the table, its neighbours, or the width dim is padded to.
 * One block per pair, TWO stores per pair, no global scratch, no atomics, no private segment.
 * CVX_EINVAL, nothing launched and the outputs untouched: a negative count; dim outside [1, CVX_DTW_MAX_DIM]; ld < dim or ld % 4 != 0;
 * frames_dev not 16-byte aligned; an item with first row < 0, frames outside [0, CVX_DTW_MAX_FRAMES] or first row + frames > n_rows; a
 * pair index outside [0, n_items); a NULL table; with n_pairs > 0 a NULL device pointer.  n_pairs == 0 is a successful call without a
 * launch.  A block whose DEVICE rows break these bounds (the device copy is not the host copy) reads no frame and stores (NaN, -1). */
#define CVX_DTW_MAX_FRAMES 4096
#define CVX_DTW_MAX_DIM 80
int cvx_dtw_f32(const float* frames_dev, int64_t n_rows, int64_t ld, int32_t dim,
                const int32_t* items_host, const int32_t* items_dev, int32_t n_items,
                const int32_t* pairs_host, const int32_t* pairs_dev, int32_t n_pairs,
                float* cost_dev, int32_t* steps_dev, cvx_stream_t s);

/* ONE NETWORK EVALUATION WITH A TIME PER SEQUENCE, and the flow-matching loss on it - csrc/flow_loss.hip.
 * Still ABI 113: three symbols and one constant added.  The conditional-flow-matching loss of held-out mels (reference acoustic.py:732-791 on
 * CoVoMix.forward(..., target = flow), :430-538) evaluates the network once with a different time for every utterance of a PACKED
 * batch (sequence i owns rows [cu[i], cu[i + 1]) of every [rows, width] tensor).  cu = int32 [n_seq + 1], given twice as the tables of
 * cvx_dtw_f32 are: the HOST copy is validated before anything is launched and sizes the launches, the DEVICE copy is what the kernels
 * search; 1 <= n_seq <= CVX_SEQ_NORM_MAX_SEQS, 0 <= cu[0], cu non-decreasing (a sequence may be empty), cu[n_seq] <= rows < 2^31.  Rows
 * outside [cu[0], cu[n_seq]) are neither read nor written.  A kernel whose DEVICE copy differs from the host copy still touches only
 * rows of that range and table rows [0, n_seq).  No copy, no allocation, no host synchronisation: graph-capturable.  All three are
 * row-local streaming kernels (one wavefront per row, the row's sequence from a wave-uniform binary search): no private segment, no
 * global scratch, no atomics (the saturation commit of a split-pair store apart).
 * CVX_EINVAL, nothing launched and every output untouched: a NULL pointer that is not optional, a bad shape, a table that breaks the
 * rules above, or what the individual entries name. */
#define CVX_SEQ_NORM_MAX_SEQS 4096
/* cvx_adarmsnorm_scaled_f32 with ONE GAMMA / BETA ROW PER SEQUENCE: row r of sequence g is normalised with gamma + g * group_stride
 * (and beta + g * group_stride; beta may be NULL) - group_stride >= D, a multiple of 4 floats, so that an [n_seq, depth, 4, D] table of
 * adaptive-norm rows is read in place.  The arithmetic per row, the fp32 output, the plain and the interleaved (y_lo == y_hi + 32,
 * D % 32 == 0) split outputs, split_scale_dev and the saturation flag are those of cvx_adarmsnorm_scaled_f32, operation for operation: a
 * sequence's rows are BIT-IDENTICAL to that entry called on the sequence's slice with its own gamma / beta row.  x, gamma, beta, y
 * 16-byte aligned, D % 4 == 0. */
int cvx_adarmsnorm_seq_f32(const float* x, const float* gamma, const float* beta, float* y, uint16_t* y_hi, uint16_t* y_lo,
                           int64_t rows, int32_t D, const int32_t* cu_host, const int32_t* cu_dev, int32_t n_seq, int64_t group_stride,
                           float scale, float eps, const float* split_scale_dev, cvx_stream_t s);
/* The inputs of the loss evaluation in one launch: with t = times_dev[g] for a row of sequence g and m = mask[row] (uint8, != 0: a
 * frame the loss counts, whose conditioning is hidden),
 *   w       [rows, dim_out]  = (1 - (1 - sigma) t) x0 + t x1       acoustic.py:773
 *   flow    [rows, dim_out]  = x1 - (1 - sigma) x0                  :775
 *   cond_in [rows, dim_cond] = m ? +0 : cond                        :469 (cond * ~mask)
 * every operation an individually rounded fp32 operation in exactly that order: a = 1 - sigma; b = a t; c = 1 - b; w = c x0 + t x1 (two
 * products, one sum); flow = x1 - a x0.  No contraction.  dim_out and dim_cond positive multiples of 4, the six row tensors 16-byte
 * aligned, 0 <= sigma <= 1.  w may be a buffer of the network (the field's input). */
int cvx_cfm_inputs_f32(const float* x1, const float* x0, const float* cond, const uint8_t* mask, const float* times_dev,
                       const int32_t* cu_host, const int32_t* cu_dev, int32_t n_seq, int64_t rows, int32_t dim_out, int32_t dim_cond,
                       float sigma, float* w, float* flow, float* cond_in, cvx_stream_t s);
/* The masked mean-squared error per sequence (acoustic.py:527-536), two launches:
 *   err_rows[r] = (sum_d (pred[r, d] - flow[r, d])^2) / dim_out       for every row of the range.  One wavefront per row: lane l sums
 *                 d = l, l + 64, ... in that order from +0, then the xor butterfly over 32, 16, 8, 4, 2, 1.
 *   num[s]      = sum of err_rows over the rows of s with mask != 0   one block per sequence: thread t sums the rows t, t + 256, ...
 *                 COUNTED FROM THE SEQUENCE'S FIRST ROW in that order from +0 (an unmasked row adds +0, whatever it holds), the
 *                 butterfly, then the four wave sums as (w0 + w1) + (w2 + w3): ceil(T / 256) + 8 additions above any term.
 *   count[s]    = the number of those rows;   loss[s] = num[s] / max((float)count[s], 1e-5f)      (an empty mask: 0)
 * All individually rounded fp32 operations, no contraction.  A sequence's loss depends on its own rows alone - not on where it sits
 * in the pool or on its neighbours.  loss fp32 [n_seq], count int32 [n_seq], err_rows fp32 [rows]. */
int cvx_masked_mse_f32(const float* pred, const float* flow, const uint8_t* mask, const int32_t* cu_host, const int32_t* cu_dev,
                       int32_t n_seq, int64_t rows, int32_t dim_out, float* err_rows, float* loss, int32_t* count, cvx_stream_t s);

/* The filter + sampling of one decode step alone (the device function cvx_t2s_decode_steps samples with; no slot state, no queue, no
 * embedding write): tokens[r] = argmax_i (kept(r, i) ? logits[r, i] / max(temperature, 1e-10) + gumbel(uniforms[r, i]) : -inf), lowest
 * index on ties, gumbel(u) = -log(-log(u)) with both logarithms clamped at 1e-20 (text2semantic.py:105-113).  logits, uniforms
 * [rows, V] fp32 with V <= 1024; filter_mode / k / thres as cvx_t2s_decoder.filter_mode / top_k / top_p; tokens int64 [rows];
 * kept NULL or uint8 [rows, V] (1 = entry passed the filter).  One thread block per row; rows do not influence each other. */
int cvx_t2s_sample_f32(const float* logits, const float* uniforms, int64_t rows, int32_t V, int32_t filter_mode, int32_t k,
                       float thres, float temperature, int64_t* tokens, uint8_t* kept, cvx_stream_t stream);

/* out[r, c] = h[r, c] * gelu(h[r, F + c]) for c < F, 0 for F <= c < ld_out   (GEGLU, text2semantic.py:154-157;
 * the encoder's feed-forward; ld_out >= F pads the K dimension of the following GEMM). */
int cvx_geglu_f32(const float* h, float* out, int64_t rows, int32_t F, int64_t ld_out, cvx_stream_t stream);

/* ------------------------------------------------------------------------
 * Operator-level entry points (the names SURVEY.md section 8(b) lists): compositions of the calls above for a C
 * caller that works operator by operator.  The Python host uses the finer-grained entry points because it fuses
 * further (RoPE into the to_qkv GEMM epilogue, the xs accumulation into the last ResBlock convolution).
 *
 * cvx_rope_attention_f32: Attention.forward between to_qkv and to_out (acoustic.py:227-235): qkv [Bt, T, 3*H*64]
 *   WITHOUT rotary embedding; half-split RoPE (:132-137; tables cos/sin [T][32]) on q and k, then the attention of
 *   cvx_attention_f32.  workspace: Bt*T*3*H*64 floats (the rotated copy).
 * cvx_hifigan_convt_f32: the ConvTranspose1d upsamplers (models.py:85-88, :103) = cvx_hifigan_conv_transpose1d_f32
 *   (the polyphase kernel the host path runs) without the max|out| side output: up = stride (> 1),
 *   pad = ksize - 1 - (ksize - up)/2, a->Wp packed by cvx_hifigan_pack_conv_transpose1d_f32.
 * cvx_hifigan_resblock_f32: ResBlock1.forward (models.py:35-42), x [B, C, L] -> out [B, C, L]:
 *   three times  x = c2(leaky_relu(c1(leaky_relu(x, .1)), .1)) + x  with dilations dil[m] (c1) and 1 (c2);
 *   the last add can also apply the generator's  xs (+)= ... / num_kernels  (accum, out_scale; models.py:104-110).
 *   x, tmp, out are three distinct buffers (x is not modified).
 * cvx_hifigan_pre_post_f32: conv_pre (models.py:81, :100; `pre`, may be NULL) and / or the output stage
 *   leaky_relu + conv_post + tanh (:112-114; post_x may be NULL) - see cvx_hifigan_post_f32. */
int cvx_rope_attention_f32(const float* qkv, const float* rope_cos, const float* rope_sin, float* out,
                           int32_t Bt, int32_t T, int32_t H, float scale, float* workspace, cvx_stream_t s);
int64_t cvx_rope_attention_workspace_floats(int32_t Bt, int32_t T, int32_t H);
int cvx_hifigan_convt_f32(const cvx_conv_args* a, cvx_stream_t s);
typedef struct {
    const float* x; int32_t B, C, L;
    const float* Wp1[3]; const float* b1[3];     /* convs1[m]: dilation dil[m]   (packed by cvx_hifigan_pack_weight_f32) */
    const float* Wp2[3]; const float* b2[3];     /* convs2[m]: dilation 1 */
    int32_t ksize; int32_t dil[3];
    float* tmp; float* out;
    const float* accum; float out_scale;         /* out = (resblock(x) (+ accum)) * out_scale; accum may alias out */
} cvx_resblock_args;
int cvx_hifigan_resblock_f32(const cvx_resblock_args* a, cvx_stream_t s);
int cvx_hifigan_pre_post_f32(const cvx_conv_args* pre, const float* post_x, const float* post_w, float post_bias,
                             float* post_y, int32_t B, int32_t C, int32_t L, float slope, cvx_stream_t s);

/* ------------------------------------------------------------------------
 * HuBERT layer-L + k-means prompt tokeniser - SURVEY.md section 8f row N4
 * (fairseq-hubert/examples/textless_nlp/gslm/speech2unit/pretrained/hubert_feature_reader.py:58-78 ->
 *  fairseq-hubert/fairseq/models/hubert/hubert.py:433-480 -> fairseq/models/wav2vec/wav2vec2.py:844-946,1078-1163,
 *  1343-1370; labels: fairseq-hubert/examples/hubert/simple_kmeans/dump_km_label.py:25-43).
 * Activations are channels-last [frames, channels] fp32 throughout, so that
 *   - conv layers 1..6 (Conv1d(C, C, k, stride), no bias, GELU) are cvx_gemm_bias_act_f32 calls over OVERLAPPING rows:
 *     A = previous layer's output, lda = stride*C, K = k*C, W repacked [C_out][k][C_in];
 *   - post_extract_proj, q|k|v, out_proj, fc1 (+GELU), fc2 (+residual) are the same GEMM, attention is
 *     cvx_attention_f32 (H = 12 heads of 64, no RoPE);
 *   - the grouped positional convolution (k = 128, 16 groups) is one GEMM per group over the packed operand below
 *     (K = k*C/groups, lda = C/groups), bias + GELU + residual in its epilogue, written back at column g*C/groups;
 *   - x.C^T of the k-means distance is a GEMM against cluster_centers_ [n_clusters, D].
 * The entry points here are the steps in between. */

/* First conv layer Conv1d(1, C, k, stride) (no bias) + GroupNorm(C, C) (per channel over all frames, biased variance)
 * + exact GELU:  out[l, c], l < L = (n_samples - k) / stride + 1.   wav2vec2.py:856-910 ("default" extractor mode).
 * workspace: cvx_hubert_conv0_workspace_floats(L, C) floats. */
int64_t cvx_hubert_conv0_workspace_floats(int64_t L, int32_t C);
int cvx_hubert_conv0_gn_gelu_f32(const float* wav, int64_t n_samples, const float* w, int32_t C, int32_t k, int32_t stride,
                                 const float* gn_gamma, const float* gn_beta, float eps,
                                 float* out, float* workspace, int64_t workspace_floats, cvx_stream_t s);

/* y[r, :] = (x[r, :] - mean) / sqrt(var + eps) * gamma + beta  (biased variance; fairseq/modules/layer_norm.py).
 * D % 4 == 0, D <= 1024; y may alias x. */
int cvx_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y,
                      int64_t rows, int32_t D, float eps, cvx_stream_t s);

/* out[g][j][c] = x[j - halo][g*D/groups + c] for halo <= j < halo + T, else 0;  out = [groups, T + 2*halo, D/groups].
 * Operand of make_conv_pos's grouped Conv1d (wav2vec2.py:925-946): output frame t of group g reads the contiguous
 * run out[g][t .. t + k - 1][:] (halo = k / 2; SamePad drops the extra last frame of an even kernel). */
int cvx_hubert_group_pack_f32(const float* x, float* out, int32_t T, int32_t D, int32_t groups, int32_t halo, cvx_stream_t s);

/* labels[t] = argmin_j ( (|x[t]|^2 - 2 * dots[t, j]) + cnorm[j] ),  dots = x . C^T  [T, K]   (dump_km_label.py:36-43;
 * ties -> lowest index).  margin (optional) receives second-best minus best distance per frame. */
int cvx_kmeans_argmin_f32(const float* x, const float* dots, const float* cnorm, int64_t* labels, float* margin,
                          int64_t T, int32_t D, int32_t K, cvx_stream_t s);

/* The whole feature extractor behind ONE call (HubertModel.extract_features(source, mask=False, output_layer),
 * hubert.py:433-480, 533-549): all launches are enqueued from C (stepping them from Python costs more host time than the
 * GPU needs).  HuBERT-Base style models: extractor_mode "default" (GroupNorm after the first conv only, no conv bias),
 * post-LN encoder layers, head dim 64.  Weights are borrowed; every cvx_linear carries the fp32 weight [N, K] (validated
 * only) and its cvx_split_f16 halves (w_hi, w_lo = halves of w / inv_scale).  conv[i] (1 <= i < n_conv) is the Conv1d
 * weight repacked [C_out][k][C_in] (K = k * C_in); pos[g] the weight-norm-folded positional conv of group g repacked
 * [C/groups][k][C/groups] with bias = the group's slice; qkv = q_proj | k_proj | v_proj stacked.  `layers` and `pos` are
 * HOST arrays.  out = [cvx_hubert_frames(m, n), dim] fp32, output of encoder layer `output_layer` (1-based, 0 = before
 * the first layer).  workspace: 256-byte aligned device memory of cvx_hubert_workspace_bytes(m, n) bytes. */
typedef struct {
    const float* w; const uint16_t* w_hi; const uint16_t* w_lo; float inv_scale;
    const float* bias;
    int32_t N, K;
} cvx_linear;
typedef struct {
    cvx_linear qkv, out, fc1, fc2;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
} cvx_hubert_layer;
typedef struct {
    int32_t n_conv; int32_t conv_k[8], conv_stride[8], conv_c[8];
    const float *conv0_w, *gn_g, *gn_b;
    cvx_linear conv[8];
    const float *ln_g, *ln_b;
    cvx_linear proj;
    int32_t dim, heads, pos_k, pos_groups;
    const cvx_linear* pos;
    const float *enc_ln_g, *enc_ln_b;
    int32_t n_layers; const cvx_hubert_layer* layers;
} cvx_hubert_model;
int32_t cvx_hubert_frames(const cvx_hubert_model* m, int64_t n_samples);
int64_t cvx_hubert_workspace_bytes(const cvx_hubert_model* m, int64_t n_samples);
int cvx_hubert_extract_features(const cvx_hubert_model* m, const float* wav, int64_t n_samples, int32_t output_layer,
                                float* out, void* workspace, int64_t workspace_bytes, cvx_stream_t s);

/* MANY UTTERANCES IN ONE CALL (ragged batch; opt-in - the one-utterance entry points above are unchanged).
 * The utterances are PACKED into one waveform: item b starts at sample S_b, a multiple of the conv stack's total hop (the product of
 * conv_stride[], 320 for HuBERT-Base), the slack in between is ZERO.  Row j of conv layer i of item b is then global row
 * S_b / (stride_0 ... stride_i) + j of ONE strided GEMM over the whole buffer; a valid row reads only valid rows of its own item, rows
 * that straddle two items are computed and never read.  The valid frames are then gathered into compact [M = sum T_b, C] rows and the
 * encoder runs on M rows: GroupNorm statistics per item, zero halos of the positional convolution per item, attention keys restricted
 * to the own item (cvx_attention_varlen_f32).  An item's features do not depend on its neighbours' samples.
 *
 * ITEM TABLE: int32 words, filled on the HOST by cvx_hubert_items_fill (cvx_hubert_items_words of them); the caller uploads a copy and
 * passes both.  n = n_items, nc = n_conv, halo = pos_k / 2:
 *   header[16]        magic, n, nc, hop, halo, M = sum T_b, Mh = M + n * 2 * halo, max T_b, packed samples (S_last + n_last), 0 ...
 *   slot[n]           S_b / hop
 *   samples[n]        n_b
 *   start[nc][n]      first global row of item b after conv layer i
 *   rows[nc][n]       its row count there (rows[nc - 1][b] = T_b = cvx_hubert_frames(m, n_b); 0 is legal)
 *   c0[n][3]          (start[0][b], rows[0][b], first GroupNorm statistics chunk of item b)
 *   cu[n + 1]         cu_seqlens over compact rows
 *   cuh[n + 1]        the same over haloed rows, cuh[b] = cu[b] + b * 2 * halo
 *   gather[M]         compact row -> global row of the last conv layer
 *   pack_src[Mh]      haloed row -> compact row, -1 in a halo
 *   unpack[M]         compact row -> haloed row where its positional-convolution output lands (cuh[b] + t)
 * cvx_hubert_items_fill: offsets == NULL packs the items tightly (every start rounded up to the hop); with offsets the caller chooses
 * S_b.  CVX_EINVAL (nothing is launched, here and in every call that takes a table) when n_items <= 0, an offset is no multiple of the
 * hop, items overlap or are out of order, or the total frame count reaches 2^24.  cvx_hubert_items_words returns -1 then.
 * cvx_hubert_extract_features_many: wav = the packed waveform of header[8] samples (slack zeroed by the caller); out = [M, dim];
 * workspace as for the one-utterance call, cvx_hubert_workspace_bytes_many bytes (-1 for an illegal table).  The host table is
 * re-derived from its slot[] / samples[] and compared word by word before anything is launched.  The positional convolution's GEMMs
 * run over all Mh - pos_k haloed rows, pos_k rows per item more than the frames. */
int64_t cvx_hubert_items_words(const cvx_hubert_model* m, const int64_t* n_samples, int32_t n_items);
int cvx_hubert_items_fill(const cvx_hubert_model* m, const int64_t* n_samples, const int64_t* offsets, int32_t n_items,
                          int32_t* table, int64_t table_words);
int64_t cvx_hubert_workspace_bytes_many(const cvx_hubert_model* m, const int32_t* items_host, int32_t n_items);
int cvx_hubert_extract_features_many(const cvx_hubert_model* m, const float* wav, const int32_t* items_host, const int32_t* items_dev,
                                     int32_t n_items, int32_t output_layer, float* out, void* workspace, int64_t workspace_bytes,
                                     cvx_stream_t s);
/* The stepping stones of the call above, each on its own.
 * cvx_hubert_conv0_gn_gelu_many_f32: the first conv layer over the whole packed waveform with GroupNorm statistics PER ITEM.
 * rows3 = n_items triples (first row, rows, first statistics chunk = sum over the items before of ceil(rows / 128)), the same words
 * in host and in device memory (the table's c0[]); items in row order, not overlapping; an item of 0 rows may start behind the last row
 * (a trailing item shorter than one stride).  out = [L, C], L = (n_samples - k) / stride + 1:
 * an item's rows normalised with its own mean / rstd (fixed-order partial sums, no atomics), every other row ZERO.
 * workspace: cvx_hubert_conv0_many_workspace_floats floats. */
int64_t cvx_hubert_conv0_many_workspace_floats(const int32_t* rows3_host, int32_t n_items, int32_t C);
int cvx_hubert_conv0_gn_gelu_many_f32(const float* wav, int64_t n_samples, const float* w, int32_t C, int32_t k, int32_t stride,
                                      const float* gn_gamma, const float* gn_beta, float eps,
                                      const int32_t* rows3_host, const int32_t* rows3_dev, int32_t n_items,
                                      float* out, float* workspace, int64_t workspace_floats, cvx_stream_t s);
/* out[r, :] = x[map[r], :] (map[r] < 0: zeros); map = `rows` int32 in device memory, C % 4 == 0. */
int cvx_row_gather_f32(const float* x, float* out, const int32_t* map_dev, int64_t rows, int32_t C, cvx_stream_t s);
/* Ragged cvx_hubert_group_pack_f32: out[g][j][c] = x[pack_src[j]][g*D/groups + c], 0 where pack_src[j] < 0 (halo rows are WRITTEN,
 * every call); out = [groups, rows, D/groups], rows = Mh, (D/groups) % 4 == 0.  Output frame t of item b of group g reads the
 * contiguous run out[g][cuh[b] + t .. + pos_k - 1][:]. */
int cvx_hubert_group_pack_many_f32(const float* x, float* out, const int32_t* pack_src_dev, int64_t rows, int32_t D, int32_t groups,
                                   cvx_stream_t s);
/* The inverse mapping with the residual: x[r, :] = h[r, :] + conv[unpack[r], :] for r < rows (= M); conv = [>= Mh - pos_k, D]. */
int cvx_hubert_group_unpack_add_f32(const float* h, const float* conv, const int32_t* unpack_dev, float* x, int64_t rows, int32_t D,
                                    cvx_stream_t s);

/* Sample-rate conversion in front of the tokeniser (hubert_feature_reader.py:38-41: torchaudio.transforms.Resample,
 * third-party; its published polyphase windowed-sinc algorithm): out[i*up + j] = sum_k kern[j][k] * x[i*down + k - width]
 * with x = 0 outside [0, n), kern = [up][2*width + down] computed by the host (covomix_amd.hubert.sinc_resample_kernel),
 * n_out = ceil(up * n / down). */
int cvx_resample_fir_f32(const float* x, int64_t n, const float* kern, int32_t up, int32_t down, int32_t width,
                         float* out, int64_t n_out, cvx_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* COVOMIX_HIP_H */
