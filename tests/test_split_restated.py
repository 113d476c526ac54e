"""The restated split-pair contract (tests/split_restated.py) against the contract's own arithmetic, on the CPU: the reference the
GPU producer tests compare bits with must itself be right.  Checked on 2^20 random values +-m * 2^e, e in [-30, 16], plus the edge
values (split_restated.SPECIALS)."""
import numpy as np

import split_restated as sr

N_RANDOM = 1 << 20


def _ladder():
    x = sr.ladder(N_RANDOM, seed=0)
    assert x.size >= 10 ** 6 and x.dtype == np.float32
    return x


def test_split_pair_difference_is_exact_and_reconstruction_is_bounded():
    x = _ladder()
    hi, lo = sr.split_pair(x)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    v = np.clip(x, -65504.0, 65504.0).astype(np.float32)
    assert np.isfinite(hi.astype(np.float64)).all() and np.isfinite(lo.astype(np.float64)).all()
    assert np.array_equal(hi.view(np.uint16), v.astype(np.float16).view(np.uint16))
    # v - hi is exact in fp32: the fp32 difference equals the fp64 difference of the same two numbers
    d32 = (v - hi.astype(np.float32)).astype(np.float32)
    d64 = v.astype(np.float64) - hi.astype(np.float64)
    assert np.array_equal(d32.astype(np.float64), d64)
    # two round-to-nearest-even roundings to 11 significant bits: |v - hi| <= 2^-11 |v| and |d - lo| <= 2^-11 |d|, i.e. 2^-22 |v|;
    # once lo is subnormal its spacing is 2^-24, so half of that.  Derived, not measured (the tie v = 2^-25 -> hi = lo = 0 reaches it).
    err = np.abs(v.astype(np.float64) - (hi.astype(np.float64) + lo.astype(np.float64)))
    bound = np.maximum(2.0 ** -22 * np.abs(v.astype(np.float64)), 2.0 ** -25)
    assert (err <= bound).all(), float((err / bound).max())
    # the distribution does reach what it is meant to: subnormal lo halves, subnormal hi halves, the clamp
    lo_abs = np.abs(lo.astype(np.float64))
    assert ((lo_abs > 0) & (lo_abs < 2.0 ** -14)).mean() > 0.1
    assert ((np.abs(hi.astype(np.float64)) > 0) & (np.abs(hi.astype(np.float64)) < 2.0 ** -14)).any()
    assert (np.abs(x) > 65504.0).any()


def test_split_pair_edges():
    def bits(x, scale=1.0):
        hi, lo = sr.split_pair(np.array([x], dtype=np.float32), scale)
        return float(hi[0]), float(lo[0])
    assert bits(65519.99) == (65504.0, 0.0) and bits(65520.0) == (65504.0, 0.0) and bits(-1e9) == (-65504.0, 0.0)   # lo of the CLAMPED value
    assert bits(2.0 ** -24) == (2.0 ** -24, 0.0) and bits(2.0 ** -25) == (0.0, 0.0) and bits(3 * 2.0 ** -26) == (2.0 ** -24, 0.0)
    assert bits(1 + 2.0 ** -11) == (1.0, 2.0 ** -11)                              # tie of the first rounding goes to even, lo carries it
    assert bits(1 + 2.0 ** -11 + 2.0 ** -23) == (1 + 2.0 ** -10, -(2.0 ** -11))           # just past the tie: hi goes up, lo's own tie (2^-23 of 2^-22) to even
    assert bits(1 + 2.0 ** -11, 2.0 ** -15) == (2.0 ** -15, 0.0)          # the difference 2^-26 is below half the subnormal spacing: lo = 0
    assert bits(3.0, 2.0 ** -3) == (0.375, 0.0)                                   # the scale is applied BEFORE the split
    hi, lo = sr.split_pair(np.array([-0.0], dtype=np.float32))
    assert hi.view(np.uint16)[0] == 0x8000 and lo.view(np.uint16)[0] == 0x0000


def test_interleave_roundtrip_and_index_map():
    rng = np.random.default_rng(1)
    for rows, cols in ((1, 32), (3, 96), (7, 160)):
        hi = rng.standard_normal((rows, cols)).astype(np.float16)
        lo = rng.standard_normal((rows, cols)).astype(np.float16)
        buf = sr.interleave(hi, lo)
        assert buf.shape == (rows, 2 * cols)
        h2, l2 = sr.deinterleave(buf, rows, cols)
        assert np.array_equal(h2, hi) and np.array_equal(l2, lo)
        # the layout IS the index map of the header
        idx = sr.il_index(np.arange(rows * cols))
        assert np.array_equal(buf.reshape(-1)[idx], hi.reshape(-1)) and np.array_equal(buf.reshape(-1)[idx + 32], lo.reshape(-1))
    for n in (32, 96, 1024):
        idx = sr.il_index(np.arange(n))
        assert np.array_equal(np.sort(np.concatenate((idx, idx + 32))), np.arange(2 * n))       # a bijection onto [0, 2n)
    assert int(sr.il_index(39)) + 32 == 103                                                        # n = 40: past 2n = 80


def test_colscale_il_and_pow2_scale():
    rng = np.random.default_rng(2)
    W = rng.standard_normal((3, 64)).astype(np.float32)
    g = rng.standard_normal((2, 64)).astype(np.float32)
    ss = np.array([0.5, 4.0], dtype=np.float32)
    out = sr.colscale_il(W, g, ss, 8.0)
    assert out.shape == (2, 3, 128) and out.dtype == np.float16
    for s in range(2):
        hi, lo = sr.deinterleave(out[s], 3, 64)
        want = (W * g[s][None, :]).astype(np.float32) * np.float32(8.0 * ss[s])
        h2, l2 = sr.split_pair(want)
        assert np.array_equal(hi.view(np.uint16), h2.view(np.uint16)) and np.array_equal(lo.view(np.uint16), l2.view(np.uint16))
    assert np.array_equal(sr.colscale_il(W, g, None, 8.0)[1], sr.colscale_il(W, g, np.ones(2, np.float32), 8.0)[1])
    assert sr.pow2_scale(0.0, 1024.0) == 1.0 and sr.pow2_scale(1.3 * 2 ** 5, 1024.0) == 2.0 ** 5      # log2(1024 / 41.6) = 4.62 -> 5
    assert sr.pow2_scale(1e-30, 1024.0) == 2.0 ** 40 and sr.pow2_scale(3e38, 1024.0) == 2.0 ** -40
    assert sr.pow2_scale(1024.0, 1024.0) == 1.0 and sr.pow2_scale(-0.0, 1.0) == 1.0
