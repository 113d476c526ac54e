"""Plain-numpy restatement of the split-pair contract (include/covomix_hip.h): what every producer of fp16 (hi, lo) pairs has
to write, bit for bit - the checker of tests/test_split_restated.py (pinned there against the contract's own error bound) and of
tests/test_split_producers_gpu.py / tests/test_rowlocal_edges_gpu.py.  Test infrastructure only: no GPU, no torch kernels.

  v  = clip(fp32(x) * fp32(scale), -65504, 65504)          (one fp32 product, then the clamp)
  hi = fp16(v)                                              round to nearest even, subnormals kept
  lo = fp16(fp32(v - fp32(hi)))                             the difference is exact in fp32; subnormals kept

Interleaved layout: a [rows, cols] pair (cols % 32 == 0) lives in ONE [rows, 2 * cols] buffer as [hi 32 | lo 32] per block of 32
columns: flat offset o of the two-tensor form sits at ((o >> 5) << 6) | (o & 31) for hi and 32 halves later for lo."""
import numpy as np

F16_MAX = np.float32(65504.0)

# the edges of the contract: signed zeros, the clamp and both sides of it (65520 is where fp16 rounding alone would reach inf), the
# smallest normal and subnormal fp16, the rounding tie below it (2^-25 -> 0, 3 * 2^-26 -> 2^-24), and two values whose lo half is a
# tie / just past a tie of the first rounding
SPECIALS = np.array([0.0, -0.0, 65504.0, -65504.0, 65519.99, 65520.0, 1e9, -1e9, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26,
                     3 * 2.0 ** -26, 1 + 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23], dtype=np.float32)


def ladder(n_random: int, seed: int = 0) -> np.ndarray:
    """SPECIALS followed by n_random values +-m * 2^e: m uniform in [1, 2), e uniform in [-30, 16] (fp32)."""
    rng = np.random.default_rng(seed)
    m = (1.0 + rng.random(n_random)).astype(np.float32)
    e = rng.integers(-30, 17, n_random)
    sign = np.where(rng.random(n_random) < 0.5, -1.0, 1.0).astype(np.float32)
    return np.concatenate((SPECIALS, (sign * np.ldexp(m, e)).astype(np.float32)))


def split_pair(x, scale=1.0):
    """(hi, lo) fp16 arrays of x * scale (see the module docstring)."""
    v = np.clip(np.asarray(x, dtype=np.float32) * np.float32(scale), -F16_MAX, F16_MAX).astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi, lo


def il_index(i):
    """Where element i (flat offset of the two-tensor form) of the hi half sits in the interleaved buffer; lo: 32 later."""
    i = np.asarray(i, dtype=np.int64)
    return ((i >> 5) << 6) | (i & 31)


def interleave(hi, lo):
    """[rows, cols] hi and lo -> [rows, 2 * cols]: [hi 32 | lo 32] per block of 32 columns."""
    rows, cols = hi.shape
    assert cols % 32 == 0 and lo.shape == hi.shape
    return np.stack((hi.reshape(rows, cols // 32, 32), lo.reshape(rows, cols // 32, 32)), axis=2).reshape(rows, 2 * cols)


def deinterleave(buf, rows: int, cols: int):
    """[rows, 2 * cols] interleaved buffer -> (hi, lo), each [rows, cols]."""
    assert cols % 32 == 0 and buf.shape == (rows, 2 * cols)
    b = buf.reshape(rows, cols // 32, 2, 32)
    return b[:, :, 0].reshape(rows, cols).copy(), b[:, :, 1].reshape(rows, cols).copy()


def colscale_il(W, colscale, set_scale, scale):
    """cvx_split_f16_colscale_il: out[s] = interleaved pair of W * colscale[s][None, :] * (scale * set_scale[s]), the products taken in
    fp32 in exactly this order ((w * g) first, then the one combined factor); set_scale None = 1.  -> fp16 [n_sets, N, 2K]."""
    W = np.asarray(W, dtype=np.float32)
    colscale = np.asarray(colscale, dtype=np.float32)
    N, K = W.shape
    n_sets = colscale.shape[0]
    out = np.empty((n_sets, N, 2 * K), dtype=np.float16)
    for s in range(n_sets):
        sc = np.float32(scale) * (np.float32(set_scale[s]) if set_scale is not None else np.float32(1.0))
        x = (W * colscale[s][None, :]).astype(np.float32) * np.float32(sc)
        out[s] = interleave(*split_pair(x))
    return out


def pow2_scale(amax, target) -> np.float32:
    """2^clip(rint(log2(target / amax)), -40, 40), and 1 for amax == 0 (cvx_amax_pow2_scale_f32 / cvx_pow2_scale_from_amax_f32)."""
    amax = float(np.float32(amax))
    if amax == 0.0:
        return np.float32(1.0)
    e = np.clip(np.rint(np.log2(float(np.float32(target)) / amax)), -40, 40)
    return np.float32(2.0 ** float(e))
