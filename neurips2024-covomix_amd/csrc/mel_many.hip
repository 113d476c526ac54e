// Prompt mel extraction of MANY wav prompts in one call (the one-prompt path is mel.py over
// cvx_gemm_bias_act_f32 + the two epilogues in elementwise.hip and stays as it is).
//   monologue_generation.py:62-74 (extract_mel) -> data_preparation/generate_mel.py:49-72 (mel_spectrogram)
// The reflect-padded signals of all items lie in ONE buffer, item b at float S_b = slot_b * hop, so that frame t of item b is row
// slot_b + t of one [R, n_fft] view with row stride hop: the windowed DFT and the mel projection are one fp32 GEMM each over all R rows.
// What is new here is what stands around the two GEMMs:
//   mel_pack_kernel        stored samples (or their polyphase FIR output) -> reflect pad -> clamp -> the packed buffer, every word written
//   mel_log_gather_kernel  proj [R, n_mels] -> log(max(., 1e-5)) of the items' own rows, transposed, item after item
// Both are HBM-bound index plumbing: 16-byte stores (and loads where the source is aligned) in the pack, coalesced stores in the gather.
// Layout of the item table: include/covomix_hip.h, "MANY PROMPTS IN ONE CALL".
#include "cvx_common.h"
#include <algorithm>
#include <string.h>

#define CVX_TRY(expr) do { const int rc_ = (expr); if (rc_ != CVX_OK) return rc_; } while (0)

namespace {

constexpr int32_t MT_MAGIC_VALUE = 0x4D454C31;        // "MEL1"
constexpr int MT_MAX_BANKS = 16;
enum { MT_MAGIC = 0, MT_N, MT_NFFT, MT_HOP, MT_PAD, MT_ROWS, MT_FRAMES, MT_MAXT, MT_PACKED, MT_RAW, MT_NBANKS, MT_BANKF, MT_HEADER = 16 };
enum { MI_RAW_OFF = 0, MI_N_RAW, MI_N, MI_SLOT, MI_T, MI_CU, MI_BANK, MI_WORDS = 8 };
enum { MB_UP = 0, MB_DOWN, MB_WIDTH, MB_OFF, MB_WORDS = 4 };

// Writes the table (out != NULL), or compares it word by word against `cmp` (validation of a caller's table: no allocation).
struct MelSink {
    int32_t* out; const int32_t* cmp; int64_t cap; bool ok;
    void put(int64_t i, int64_t v)
    {
        if (i >= cap) { ok = false; return; }
        if (out) out[i] = (int32_t)v;
        else if (cmp && cmp[i] != (int32_t)v) ok = false;
    }
};

// The one place the layout is computed.  Inputs are the caller's arrays, or (from_table != NULL, of `cap` words) the n_raw / bank words
// and the bank geometry of a table.  Returns the table's word count, -1 when the items are not a legal batch.
int64_t build_mel_items(int64_t n_fft, int64_t hop, const int64_t* n_raw, const int32_t* bank, const int32_t* bank_geom, int64_t n_banks,
                        const int32_t* from_table, int64_t n_items, MelSink sink)
{
    constexpr int64_t LIM = (int64_t)1 << 31;
    if (n_items <= 0 || n_items >= (1 << 24) || n_banks < 0 || n_banks > MT_MAX_BANKS) return -1;
    if (n_fft <= 0 || hop <= 0 || n_fft >= (1 << 20) || n_fft % 4 || hop % 4 || hop > n_fft || (n_fft - hop) % 2) return -1;
    const int64_t words = MT_HEADER + MI_WORDS * n_items + MB_WORDS * n_banks;
    if (from_table && sink.cap < words) return -1;
    const int64_t pad = (n_fft - hop) / 2;
    const int64_t banks_at = MT_HEADER + MI_WORDS * n_items;
    int64_t b_up[MT_MAX_BANKS], b_down[MT_MAX_BANKS], b_width[MT_MAX_BANKS], b_off[MT_MAX_BANKS], bank_floats = 0;
    for (int64_t j = 0; j < n_banks; ++j) {
        const int32_t* g = from_table ? from_table + banks_at + MB_WORDS * j : bank_geom + 3 * j;
        b_up[j] = g[0]; b_down[j] = g[1]; b_width[j] = g[2];
        if (b_up[j] <= 0 || b_down[j] <= 0 || b_width[j] < 0 || b_up[j] >= (1 << 20) || b_down[j] >= (1 << 20) || b_width[j] >= (1 << 20)) return -1;
        b_off[j] = bank_floats;
        bank_floats += b_up[j] * (2 * b_width[j] + b_down[j]);
        if (bank_floats >= LIM) return -1;
    }
    auto raw_of = [&](int64_t b) -> int64_t { return from_table ? from_table[MT_HEADER + MI_WORDS * b + MI_N_RAW] : n_raw[b]; };
    auto bank_of = [&](int64_t b) -> int64_t { return from_table ? from_table[MT_HEADER + MI_WORDS * b + MI_BANK] : (bank ? bank[b] : -1); };
    if (!sink.out && !sink.cmp) sink.cap = 0;                        // only counting: put() writes nothing and `ok` is not looked at
    else if (sink.cap < words) return -1;
    int64_t raw_off = 0, slot = 0, cu = 0, maxT = 0;
    for (int64_t b = 0; b < n_items; ++b) {
        const int64_t nr = raw_of(b), bk = bank_of(b);
        if (nr < 0 || nr >= LIM || bk < -1 || bk >= n_banks) return -1;
        const int64_t nb = bk < 0 ? nr : (b_up[bk] * nr + b_down[bk] - 1) / b_down[bk];
        if (nb <= pad || nb < 1 || nb >= LIM) return -1;             // the reflection needs pad < n_b
        const int64_t L = nb + 2 * pad;
        const int64_t T = L < n_fft ? 0 : (L - n_fft) / hop + 1;
        const int64_t at = MT_HEADER + MI_WORDS * b;
        sink.put(at + MI_RAW_OFF, raw_off); sink.put(at + MI_N_RAW, nr); sink.put(at + MI_N, nb); sink.put(at + MI_SLOT, slot);
        sink.put(at + MI_T, T); sink.put(at + MI_CU, cu); sink.put(at + MI_BANK, bk); sink.put(at + 7, 0);
        raw_off = (raw_off + nr + 3) / 4 * 4;
        slot += (L + hop - 1) / hop;
        cu += T; maxT = std::max(maxT, T);
        if (raw_off >= LIM || slot * hop + n_fft >= LIM || cu >= (1 << 24)) return -1;
    }
    const int64_t packed = (slot * hop + n_fft - hop + 3) / 4 * 4;
    for (int i = MT_BANKF + 1; i < MT_HEADER; ++i) sink.put(i, 0);
    sink.put(MT_MAGIC, MT_MAGIC_VALUE); sink.put(MT_N, n_items); sink.put(MT_NFFT, n_fft); sink.put(MT_HOP, hop); sink.put(MT_PAD, pad);
    sink.put(MT_ROWS, slot); sink.put(MT_FRAMES, cu); sink.put(MT_MAXT, maxT); sink.put(MT_PACKED, packed); sink.put(MT_RAW, raw_off);
    sink.put(MT_NBANKS, n_banks); sink.put(MT_BANKF, bank_floats);
    for (int64_t j = 0; j < n_banks; ++j) {
        const int64_t at = banks_at + MB_WORDS * j;
        sink.put(at + MB_UP, b_up[j]); sink.put(at + MB_DOWN, b_down[j]); sink.put(at + MB_WIDTH, b_width[j]); sink.put(at + MB_OFF, b_off[j]);
    }
    if ((sink.out || sink.cmp) && !sink.ok) return -1;
    return words;
}

// A caller's host table: re-derived from its own words and compared word by word.
int check_host_table(const int32_t* items, int64_t items_words, int32_t n_items, const char* who)
{
    CVX_REQUIRE(items && n_items > 0 && items_words >= MT_HEADER + (int64_t)MI_WORDS * n_items, "%s: no item table of %d items", who, n_items);
    const int64_t words = build_mel_items(items[MT_NFFT], items[MT_HOP], nullptr, nullptr, nullptr, items[MT_NBANKS], items, n_items,
                                          MelSink{nullptr, items, items_words, true});
    CVX_REQUIRE(words > 0 && words == items_words && items[MT_N] == n_items, "%s: the host item table is not the table cvx_mel_items_fill "
                "writes for %d items (%ld words)", who, n_items, (long)items_words);
    return CVX_OK;
}

// The device copy, read back in pieces into the stack (blocking; nothing has been launched yet) and compared with the host copy.
int check_device_table(const int32_t* items_host, const int32_t* items_dev, int64_t items_words, hipStream_t st, const char* who)
{
    CVX_REQUIRE(items_dev, "%s: no device copy of the item table", who);
    int32_t buf[2048];
    for (int64_t at = 0; at < items_words; at += 2048) {
        const int64_t n = std::min<int64_t>(2048, items_words - at);
        if (hipMemcpyAsync(buf, items_dev + at, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            (void)hipGetLastError();
            cvx_set_error("%s: the device copy of the item table cannot be read", who);
            return CVX_EHIP;
        }
        CVX_REQUIRE(memcmp(buf, items_host + at, (size_t)n * sizeof(int32_t)) == 0, "%s: the device copy of the item table differs from the "
                    "host copy (words %ld..%ld)", who, (long)at, (long)(at + n - 1));
    }
    return CVX_OK;
}

// last item whose first slot is <= slot (item 0 starts at slot 0)
__device__ __forceinline__ int mel_item_of_slot(const int32_t* __restrict__ items, int n_items, int slot)
{
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid * MI_WORDS + MI_SLOT] <= slot) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One output sample of the polyphase resampler: the loop of resample_fir_kernel (hubert.hip) restated - same taps, same fmaf order,
// x = 0 outside [0, n) - so that a resampled item is bit for bit resample -> clamp -> pad.
__device__ __forceinline__ float mel_fir_at(const float* __restrict__ x, int64_t n, const float* __restrict__ kern, int64_t o,
                                            int up, int down, int width, int kw)
{
    const int64_t i = o / up;
    const int j = (int)(o % up);
    const int64_t base = i * down - width;
    const float* kj = kern + (int64_t)j * kw;
    float acc = 0.f;
    for (int k = 0; k < kw; ++k) {
        const int64_t p = base + k;
        if (p >= 0 && p < n) acc = fmaf(kj[k], x[p], acc);
    }
    return acc;
}

// torch.clamp(v, -1, 1): a NaN stays a NaN
__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }

// thread = 4 consecutive floats of the packed buffer (hop % 4 == 0: they lie in one slot, so in one item).  The last item owns the tail.
__global__ __launch_bounds__(256) void mel_pack_kernel(const float* __restrict__ raw, const float* __restrict__ banks,
                                                      const int32_t* __restrict__ table, int n_items, int hop, int pad, int64_t packed4,
                                                      float* __restrict__ packed)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= packed4) return;
    const int64_t p0 = i * 4;
    const int32_t* items = table + MT_HEADER;
    const int32_t* it = items + mel_item_of_slot(items, n_items, (int)(p0 / hop)) * MI_WORDS;
    const int64_t q0 = p0 - (int64_t)it[MI_SLOT] * hop;               // position in the item's padded signal
    const int64_t nb = it[MI_N], nr = it[MI_N_RAW];
    const int bank = it[MI_BANK];
    const float* x = raw + it[MI_RAW_OFF];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int64_t j0 = q0 - pad;
    if (bank < 0 && j0 >= 0 && j0 + 3 < nb && ((it[MI_RAW_OFF] + j0) & 3) == 0) {      // interior of a stored signal, 16-byte aligned
        v = gload4(x + j0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = clamp1(v[e]);
    } else if (q0 < nb + 2 * pad) {
        int up = 1, down = 1, width = 0;
        const float* kern = nullptr;
        if (bank >= 0) {
            const int32_t* bk = items + (int64_t)n_items * MI_WORDS + bank * MB_WORDS;
            up = bk[MB_UP]; down = bk[MB_DOWN]; width = bk[MB_WIDTH];
            kern = banks + bk[MB_OFF];
        }
        const int kw = 2 * width + down;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (q0 + e >= nb + 2 * pad) continue;                     // slack behind the item: zero
            int64_t j = j0 + e;
            j = j < 0 ? -j : (j >= nb ? 2 * (nb - 1) - j : j);        // reflect (pad < n_b: one reflection is enough)
            v[e] = clamp1(bank < 0 ? x[j] : mel_fir_at(x, nr, kern, j, up, down, width, kw));
        }
    }
    *reinterpret_cast<f32x4*>(packed + p0) = v;
}

// thread = one output float.  Items of no frames share their cu with the next item: the search takes the LAST item whose cu is <= the
// output frame, which is the one that owns it.
__global__ __launch_bounds__(256) void mel_log_gather_kernel(const float* __restrict__ proj, const int32_t* __restrict__ table, int n_items,
                                                            int n_mels, int64_t total, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int32_t* items = table + MT_HEADER;
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)items[mid * MI_WORDS + MI_CU] * n_mels <= i) lo = mid; else hi = mid - 1;
    }
    const int32_t* it = items + lo * MI_WORDS;
    const int64_t T = it[MI_T];
    const int64_t j = i - (int64_t)it[MI_CU] * n_mels;
    const int64_t m = j / T, t = j - m * T;
    out[i] = logf(fmaxf(proj[((int64_t)it[MI_SLOT] + t) * n_mels + m], 1e-5f));
}

struct MelPlanMany {
    int64_t R, M, packed;
    int n_fft, hop, pad, nb, nbp;
    float *sig, *spec, *mag, *proj;
    int64_t bytes;
};

int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }

void plan_mel_many(const int32_t* items, int32_t n_mels, void* ws, MelPlanMany& P)
{
    P.R = items[MT_ROWS]; P.M = items[MT_FRAMES]; P.packed = items[MT_PACKED];
    P.n_fft = items[MT_NFFT]; P.hop = items[MT_HOP]; P.pad = items[MT_PAD];
    P.nb = P.n_fft / 2 + 1; P.nbp = (P.nb + 3) / 4 * 4;
    char* base = reinterpret_cast<char*>(ws);
    int64_t off = 0;
    auto take = [&](int64_t floats) { float* p = reinterpret_cast<float*>(base + off); off += up256(floats * (int64_t)sizeof(float)); return p; };
    P.sig = take(P.packed);
    P.spec = take(P.R * 2 * P.nb);
    P.mag = take(P.R * P.nbp);
    P.proj = take(P.R * n_mels);
    P.bytes = off;
}

int launch_pack(const float* raw, const float* banks, const int32_t* items_host, const int32_t* items_dev, int32_t n_items, float* packed,
                hipStream_t st)
{
    const int64_t packed4 = items_host[MT_PACKED] / 4;
    hipLaunchKernelGGL(mel_pack_kernel, dim3((unsigned)((packed4 + 255) / 256)), dim3(256), 0, st, raw, banks, items_dev, n_items,
                       items_host[MT_HOP], items_host[MT_PAD], packed4, packed);
    CVX_CHECK_LAUNCH("cvx_mel_pack_f32");
    return CVX_OK;
}

int launch_log_gather(const float* proj, const int32_t* items_host, const int32_t* items_dev, int32_t n_items, int32_t n_mels, float* out,
                      hipStream_t st)
{
    const int64_t total = (int64_t)items_host[MT_FRAMES] * n_mels;
    if (total == 0) return CVX_OK;
    hipLaunchKernelGGL(mel_log_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, proj, items_dev, n_items, n_mels,
                       total, out);
    CVX_CHECK_LAUNCH("cvx_mel_log_gather_f32");
    return CVX_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int64_t cvx_mel_items_words(int32_t n_fft, int32_t hop, const int64_t* n_raw, const int32_t* bank, const int32_t* bank_geom,
                                       int32_t n_banks, int32_t n_items)
{
    if (!n_raw || (n_banks > 0 && !bank_geom)) return -1;
    return build_mel_items(n_fft, hop, n_raw, bank, bank_geom, n_banks, nullptr, n_items, MelSink{nullptr, nullptr, 0, true});
}

extern "C" int cvx_mel_items_fill(int32_t n_fft, int32_t hop, const int64_t* n_raw, const int32_t* bank, const int32_t* bank_geom,
                                  int32_t n_banks, int32_t n_items, int32_t* table, int64_t table_words)
{
    CVX_REQUIRE(n_raw && table && n_items > 0 && (n_banks <= 0 || bank_geom), "mel_items_fill: bad arguments");
    // counted first: an illegal batch leaves the caller's table untouched
    const int64_t need = build_mel_items(n_fft, hop, n_raw, bank, bank_geom, n_banks, nullptr, n_items, MelSink{nullptr, nullptr, 0, true});
    CVX_REQUIRE(need > 0 && need <= table_words, "mel_items_fill: not a legal batch (n_fft %d, hop %d: multiples of 4, hop <= n_fft, n_fft - hop "
                "even; every item longer than (n_fft - hop) / 2 samples at the target rate and naming a bank of the call or -1; packed "
                "buffer, raw samples and banks within int32, fewer than 2^24 frames; the table large enough)", n_fft, hop);
    const int64_t words = build_mel_items(n_fft, hop, n_raw, bank, bank_geom, n_banks, nullptr, n_items, MelSink{table, nullptr, table_words, true});
    CVX_REQUIRE(words == need, "mel_items_fill: internal error");
    return CVX_OK;
}

extern "C" int cvx_mel_pack_f32(const float* raw, const float* banks, const int32_t* items_host, const int32_t* items_dev, int64_t items_words,
                                int32_t n_items, float* packed, cvx_stream_t s)
{
    CVX_TRY(check_host_table(items_host, items_words, n_items, "mel_pack"));
    CVX_REQUIRE(raw && packed && aligned16(raw) && aligned16(packed), "mel_pack: raw / packed (16-byte aligned)");
    CVX_REQUIRE(banks || items_host[MT_NBANKS] == 0, "mel_pack: the table names %d filter banks and `banks` is NULL", items_host[MT_NBANKS]);
    CVX_TRY(check_device_table(items_host, items_dev, items_words, cvx_hip_stream(s), "mel_pack"));
    return launch_pack(raw, banks, items_host, items_dev, n_items, packed, cvx_hip_stream(s));
}

extern "C" int cvx_mel_log_gather_f32(const float* proj, const int32_t* items_host, const int32_t* items_dev, int64_t items_words,
                                      int32_t n_items, int32_t n_mels, float* out, cvx_stream_t s)
{
    CVX_TRY(check_host_table(items_host, items_words, n_items, "mel_log_gather"));
    CVX_REQUIRE(n_mels > 0 && (int64_t)items_host[MT_FRAMES] * n_mels < ((int64_t)1 << 31), "mel_log_gather: n_mels %d", n_mels);
    CVX_REQUIRE(proj && (out || items_host[MT_FRAMES] == 0), "mel_log_gather: null pointer");
    CVX_TRY(check_device_table(items_host, items_dev, items_words, cvx_hip_stream(s), "mel_log_gather"));
    return launch_log_gather(proj, items_host, items_dev, n_items, n_mels, out, cvx_hip_stream(s));
}

extern "C" int64_t cvx_mel_workspace_bytes_many(const int32_t* items_host, int64_t items_words, int32_t n_items, int32_t n_mels)
{
    if (n_mels <= 0 || check_host_table(items_host, items_words, n_items, "mel_workspace_bytes_many") != CVX_OK) return -1;
    MelPlanMany P{};
    plan_mel_many(items_host, n_mels, nullptr, P);
    return P.bytes;
}

extern "C" int cvx_mel_spectrogram_many_f32(const float* raw, const float* banks, const float* dft, const float* basis, int32_t n_mels,
                                            const int32_t* items_host, const int32_t* items_dev, int64_t items_words, int32_t n_items,
                                            float* out, void* workspace, int64_t workspace_bytes, cvx_stream_t s)
{
    CVX_TRY(check_host_table(items_host, items_words, n_items, "mel_spectrogram_many"));
    CVX_REQUIRE(n_mels > 0 && (int64_t)items_host[MT_FRAMES] * n_mels < ((int64_t)1 << 31), "mel_spectrogram_many: n_mels %d", n_mels);
    CVX_REQUIRE(raw && dft && basis && aligned16(raw) && aligned16(dft) && aligned16(basis), "mel_spectrogram_many: raw / dft / basis (16-byte aligned)");
    CVX_REQUIRE(banks || items_host[MT_NBANKS] == 0, "mel_spectrogram_many: the table names %d filter banks and `banks` is NULL", items_host[MT_NBANKS]);
    MelPlanMany P{};
    plan_mel_many(items_host, n_mels, workspace, P);
    CVX_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && workspace_bytes >= P.bytes,
                "mel_spectrogram_many: workspace (256-byte aligned, %ld bytes; %ld given)", (long)P.bytes, (long)workspace_bytes);
    CVX_REQUIRE(out || P.M == 0, "mel_spectrogram_many: out is NULL");
    hipStream_t st = cvx_hip_stream(s);
    CVX_TRY(check_device_table(items_host, items_dev, items_words, st, "mel_spectrogram_many"));
    if (P.M == 0) return CVX_OK;                          // every padded item is shorter than one window: nothing to write
    CVX_TRY(launch_pack(raw, banks, items_host, items_dev, n_items, P.sig, st));
    cvx_gemm_args g{};
    g.A = P.sig; g.lda = P.hop;                           // overlapping rows: frame r = sig[hop r : hop r + n_fft]
    g.W = dft; g.ldw = P.n_fft;
    g.C = P.spec; g.ldc = 2 * P.nb;
    g.M = (int32_t)P.R; g.N = 2 * P.nb; g.K = P.n_fft; g.act = CVX_ACT_NONE;
    CVX_TRY(cvx_gemm_bias_act_f32(&g, s));
    CVX_TRY(cvx_mel_magnitude_f32(P.spec, P.mag, P.R, P.nb, P.nbp, s));
    cvx_gemm_args h{};
    h.A = P.mag; h.lda = P.nbp;
    h.W = basis; h.ldw = P.nbp;
    h.C = P.proj; h.ldc = n_mels;
    h.M = (int32_t)P.R; h.N = n_mels; h.K = P.nbp; h.act = CVX_ACT_NONE;
    CVX_TRY(cvx_gemm_bias_act_f32(&h, s));
    return launch_log_gather(P.proj, items_host, items_dev, n_items, n_mels, out, st);
}
