"""Every producer of fp16 (hi, lo) split pairs against the restated contract (tests/split_restated.py), BIT FOR BIT: the uint16
views of what the kernel wrote must equal the numpy restatement's.  IEEE round-to-nearest-even leaves no freedom here: the build
passes no flush-to-zero / fast-math flag, every product the kernels take before the split is a single correctly rounded fp32
multiply, and the clamp sits between the product and the subtraction (nothing can be contracted into an fma).

Which case catches which wrong producer:
  * lo flushed to zero below 2^-14 ......... every in-range case: the ladder holds 2^-24, 3 * 2^-26, 1 + 2^-11 + 2^-23 and random values
                                             down to 2^-30, about a quarter of whose lo halves are subnormal (n >= 31 reaches them)
  * lo computed from the unclamped value ... test_above_the_clamp (65519.99 -> hi 65504, lo must be 0, not 16)
  * hi and lo blocks swapped (interleaved) . the SplitIL cases of test_split_act_f16_interleaved / test_adarmsnorm_split_outputs and
                                             test_split_f16_colscale_il (compared with split_restated.interleave)
  * last partial group of 4 / 256 skipped .. n = 1, 31, 255, 257, 256 * 7 + 5 (buffers are prefilled with a NaN pattern), N * K / 4 not a
                                             multiple of 256, D = 288 / 544 / 1056, the channels-last buffer of 4 * (256 * 3 + 1) elements
  * scale applied after the split .......... host scale 2^-3, device scale 2^5, split_scale 2^3, z_scale 2^-2: scaling a finished pair
                                             rounds at other places (and leaves other subnormals) than splitting the scaled value

NaN stays out (tests/test_saturation_gpu.py owns the flag for it).  Values above 65504 have a case of their own that also expects the
saturation flag; every other case expects it clear."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_restated as sr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN16 = 0x7E00                    # prefill of every fp16 buffer: a store that is skipped or misplaced leaves / destroys it
LADDER = sr.ladder(8192, seed=3)  # shared by all cases, built once


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import covomix_amd.ops as o
    return o


def in_range(n, total_scale=1.0, limit=65504.0):
    """The first n ladder values that stay inside the clamp after the pre-scale (specials first)."""
    x = LADDER[np.abs(LADDER.astype(np.float64) * total_scale) <= limit]
    assert x.size >= n
    return x[:n].copy()


def u16(t) -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint16)


def f16_buffer(n):
    return torch.full((n,), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)


def one(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device=DEV)


def clean(ops):
    """with clean(ops): ... - the saturation flag is clear before and must still be clear after."""
    class _Guard:
        def __enter__(self):
            ops.saturation_reset()

        def __exit__(self, et, ev, tb):
            if et is None:
                assert ops.saturation_query() == 0, "an in-range case raised the saturation flag"
            return False
    return _Guard()


def split_dev(ops, x, hi, lo, n, host_scale, dev_scale):
    """cvx_split_f16_dev through the C ABI the way ops.split_act_f16 calls it, with a host scale of the caller's choice."""
    from covomix_amd import _lib
    ops.ensure_saturation_bound()
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
    _lib.check(_lib.load().cvx_split_f16_dev(x.data_ptr(), ptr(hi), ptr(lo), n, host_scale, ops._sp(dev_scale), ops._stream()), "cvx_split_f16_dev")


# ---------------------------------------------------------------- cvx_split_f16[_dev]
@pytest.mark.parametrize("host_scale,dev_scale", [(1.0, None), (2.0 ** -3, None), (1.0, 2.0 ** 5), (2.0 ** -3, 2.0 ** 5)])
@pytest.mark.parametrize("n", [1, 31, 255, 256, 257, 256 * 7 + 5])
def test_split_act_f16_pair_and_hi_only(ops, n, host_scale, dev_scale):
    """One thread per element in blocks of 256: below, at and past a block, and a last block of five.  Plain pair and hi-only."""
    total = host_scale * (dev_scale or 1.0)
    xs = in_range(n, total)
    x = torch.from_numpy(xs).to(DEV)
    want_hi, want_lo = sr.split_pair(xs, total)
    pad = 64
    for with_lo in (True, False):
        hi, lo = f16_buffer(n + pad), (f16_buffer(n + pad) if with_lo else None)
        with clean(ops):
            if host_scale == 1.0:
                ops.split_act_f16(x, hi, lo, scale=one(dev_scale))
            else:
                split_dev(ops, x, hi, lo, n, host_scale, one(dev_scale))
        assert np.array_equal(u16(hi)[:n], u16(want_hi))
        assert (u16(hi)[n:] == NAN16).all()
        if with_lo:
            assert np.array_equal(u16(lo)[:n], u16(want_lo))
            assert (u16(lo)[n:] == NAN16).all()
    if host_scale == 1.0 and dev_scale is None:              # the allocating form of the front end
        with clean(ops):
            hi, lo = ops.split_act_f16(x)
        assert np.array_equal(u16(hi), u16(want_hi)) and np.array_equal(u16(lo), u16(want_lo))


@pytest.mark.parametrize("host_scale,dev_scale", [(1.0, None), (1.0, 2.0 ** 5), (2.0 ** -3, 2.0 ** 5)])
@pytest.mark.parametrize("rows,cols", [(1, 32), (9, 32), (3, 96), (19, 96)])
def test_split_act_f16_interleaved(ops, rows, cols, host_scale, dev_scale):
    """A SplitIL: one and three blocks of 32 per row, less than a block of 256 threads and more than one."""
    total = host_scale * (dev_scale or 1.0)
    xs = in_range(rows * cols, total).reshape(rows, cols)
    il = ops.SplitIL(rows, cols, DEV)
    il.buf.view(torch.int16).fill_(NAN16)
    x = torch.from_numpy(xs).to(DEV)
    with clean(ops):
        if host_scale == 1.0:
            ops.split_act_f16(x, il, scale=one(dev_scale))
        else:
            split_dev(ops, x, il.buf.data_ptr(), il.buf.data_ptr() + 64, rows * cols, host_scale, one(dev_scale))
    want = sr.interleave(*sr.split_pair(xs, total))
    assert np.array_equal(u16(il.buf), u16(want))
    hi, lo = il.dense()
    assert np.array_equal(u16(hi), u16(sr.deinterleave(want, rows, cols)[0])) and np.array_equal(u16(lo), u16(sr.deinterleave(want, rows, cols)[1]))


def test_split_f16_own_scale(ops):
    """split_f16(w) picks its own power of two: max|hi| lands in [2^13, 2^14), the pair is the restated split of w * scale, and
    (hi + lo) / scale gives w back within the contract's bound."""
    xs = in_range(1500, 1.0, limit=64.0)
    xs[700] = 77.7                                            # the maximum, and no power of two
    w = torch.from_numpy(xs.reshape(30, 50)).to(DEV)
    with clean(ops):
        hi, lo, inv = ops.split_f16(w)
    scale = 1.0 / inv
    assert scale == 2.0 ** 7                                  # 77.7 * 2^7 = 9945.6 in [2^13, 2^14)
    h64, l64 = hi.double().cpu().numpy().reshape(-1), lo.double().cpu().numpy().reshape(-1)
    assert 2.0 ** 13 <= np.abs(h64).max() < 2.0 ** 14
    want_hi, want_lo = sr.split_pair(xs, scale)
    assert np.array_equal(u16(hi).reshape(-1), u16(want_hi)) and np.array_equal(u16(lo).reshape(-1), u16(want_lo))
    v = xs.astype(np.float64) * scale
    assert (np.abs(v - (h64 + l64)) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all()
    assert (np.abs(xs.astype(np.float64) - inv * (h64 + l64)) <= inv * np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all()
    with clean(ops):
        hi1, lo1, inv1 = ops.split_f16(w, with_lo=False)
    assert lo1 is None and inv1 == inv and np.array_equal(u16(hi1), u16(hi))


# ---------------------------------------------------------------- cvx_split_f16_colscale_il
@pytest.mark.parametrize("n_sets,strided_set_scale", [(1, False), (3, True)])
@pytest.mark.parametrize("N,K", [(5, 96), (1, 32), (9, 160)])
def test_split_f16_colscale_il(ops, N, K, n_sets, strided_set_scale):
    """N * K / 4 is no multiple of 256 (N = 1: eight threads); W is a column slice (ldw > K), colscale a slice of a wider tensor
    (cs_ld > K), set_scale absent or a strided view; the halves behind the last set's last row must survive."""
    rng = np.random.default_rng(N * 1000 + K + n_sets)
    wide = np.zeros((N, K + 8), dtype=np.float32)
    wide[:, 4:4 + K] = in_range(N * K, 1.0, limit=2.0 ** 12).reshape(N, K)
    cs_wide = rng.uniform(-1.0, 1.0, (n_sets, K + 12)).astype(np.float32)
    ss_wide = np.zeros((n_sets, 3), dtype=np.float32)
    ss_wide[:, 1] = [0.5, 2.0, 0.25][:n_sets]
    scale = 4.0                                                # |w * g * scale * set_scale| <= 2^12 * 1 * 4 * 2 = 2^15: in range
    wd, csd, ssd = (torch.from_numpy(a).to(DEV) for a in (wide, cs_wide, ss_wide))
    w, cs = wd[:, 4:4 + K], csd[:, 4:4 + K]
    ss = ssd[:, 1] if strided_set_scale else None
    assert w.stride(0) > K and cs.stride(0) > K and (ss is None or ss.stride(0) == 3)
    total = n_sets * N * 2 * K
    buf = f16_buffer(total + 64)
    with clean(ops):
        ops.split_f16_colscale_il(w, cs, ss, scale, buf[:total].view(n_sets, N, 2 * K))
    want = sr.colscale_il(wide[:, 4:4 + K], cs_wide[:, 4:4 + K], ss_wide[:, 1] if strided_set_scale else None, scale)
    got = u16(buf)
    assert np.array_equal(got[:total].reshape(n_sets, N, 2 * K), u16(want))
    assert (got[total:] == NAN16).all()


# ---------------------------------------------------------------- the split outputs of cvx_adarmsnorm_scaled_f32
def _norm_ref(x, gamma, beta, rpg):
    D = x.shape[-1]
    g = torch.arange(x.shape[0]) // rpg
    ref = F.normalize(x.double(), dim=-1) * D ** 0.5 * gamma.double()[g]
    return ref + beta.double()[g] if beta is not None else ref


NORM_CONFIGS = [              # rows, rows_per_group, gamma rows, beta, split_scale, all-zero row
    (1, None, 1, True, None, None),
    (5, None, 1, False, 2.0 ** 3, None),
    (10, 4, 3, True, 2.0 ** 3, 6),
    (10, 4, 3, False, None, 9),
]


@pytest.mark.parametrize("rows,rpg,n_gamma,with_beta,split_scale,zero_row", NORM_CONFIGS)
@pytest.mark.parametrize("D", [32, 256, 288, 512, 544, 1024, 1056, 2048])
def test_adarmsnorm_split_outputs(ops, D, rows, rpg, n_gamma, with_beta, split_scale, zero_row):
    """Each adarmsnorm_kernel<NV> instance full (D = 256, 512, 1024) and with a partly filled last lane group (32, 288, 544), the
    first D of the two-pass kernel (1056) and 2048; 1, 5 and 10 rows (idle waves in the last block of four); groups of 4 rows over
    10 rows (a partial last group); without beta; an all-zero row.  fp32 output vs fp64 row by row; the split copy is the restated
    split of the kernel's OWN fp32 output times split_scale (same register value: exact whatever the summation order); a split-only
    call writes the same bits."""
    g = torch.Generator().manual_seed(D * 16 + rows)
    x = torch.randn(rows, D, generator=g)
    if zero_row is not None:
        x[zero_row] = 0.0
    gamma = torch.randn(n_gamma, D, generator=g)
    gamma[:, ::7] *= 2.0 ** -14                               # columns whose hi halves are fp16 subnormals too
    beta = torch.randn(n_gamma, D, generator=g) if with_beta else None
    if beta is not None:
        beta[:, ::7] *= 2.0 ** -14
    xd, gd, bd = x.to(DEV), gamma.to(DEV), (beta.to(DEV) if beta is not None else None)
    ref = _norm_ref(x, gamma, beta, rpg or rows)
    ss = split_scale or 1.0

    def targets(kind):
        if kind == "il":
            il = ops.SplitIL(rows, D, DEV)
            il.buf.view(torch.int16).fill_(NAN16)
            return il, lambda: il.buf
        hi = f16_buffer(rows * D + 64)
        lo = f16_buffer(rows * D + 64) if kind == "pair" else None
        return (hi[:rows * D].view(rows, D), lo[:rows * D].view(rows, D) if lo is not None else None), lambda: (hi, lo)

    for kind in ("pair", "hi_only", "il"):
        out = torch.full((rows, D), float("nan"), device=DEV)
        tgt, raw = targets(kind)
        with clean(ops):
            ops.adarmsnorm(xd, gd, bd, out, rows_per_group=rpg, out_split=tgt, split_scale=one(split_scale))
        o = out.cpu()
        for r in range(rows):
            if r == zero_row:                                  # 0 * (scale / eps) * gamma: exactly beta (or zero); no ratio against a zero row
                want = beta[r // rpg] if beta is not None else torch.zeros(D)
                assert torch.equal(o[r], want), f"zero row {r}"
            else:
                e = rel_l2(o[r], ref[r])
                assert e < 2e-6, f"row {r}: rel_l2 {e:.3e}"
        want_hi, want_lo = sr.split_pair(o.numpy(), ss)
        tgt2, raw2 = targets(kind)
        with clean(ops):
            ops.adarmsnorm(xd, gd, bd, None, rows_per_group=rpg, out_split=tgt2, split_scale=one(split_scale))
        for what, buf in (("with out", raw()), ("split only", raw2())):
            if kind == "il":
                assert np.array_equal(u16(buf), u16(sr.interleave(want_hi, want_lo))), what
                continue
            hi, lo = buf
            assert np.array_equal(u16(hi)[:rows * D].reshape(rows, D), u16(want_hi)), what
            assert (u16(hi)[rows * D:] == NAN16).all(), what
            if kind == "pair":
                assert np.array_equal(u16(lo)[:rows * D].reshape(rows, D), u16(want_lo)), what
                assert (u16(lo)[rows * D:] == NAN16).all(), what


# ---------------------------------------------------------------- cvx_hifigan_split_channels_last
@pytest.mark.parametrize("z_scale", [None, 2.0 ** -2])
def test_hifigan_split_channels_last(ops, z_scale):
    """4 * (256 * 3 + 1) elements: the grid-stride loop over groups of four ends one group into its fourth block."""
    n = 4 * (256 * 3 + 1)
    zs = z_scale or 1.0
    xs = in_range(n, zs).reshape(1, n // 4, 4)
    zh, zl = f16_buffer(n + 64), f16_buffer(n + 64)
    with clean(ops):
        ops.hifigan_split_channels_last(torch.from_numpy(xs).to(DEV), (zh[:n].view(xs.shape), zl[:n].view(xs.shape)), 0.1, z_scale=one(z_scale))
    act = np.where(xs > 0, xs, xs * np.float32(0.1)).astype(np.float32)
    want_hi, want_lo = sr.split_pair(act, zs)
    assert np.array_equal(u16(zh)[:n], u16(want_hi).reshape(-1)) and np.array_equal(u16(zl)[:n], u16(want_lo).reshape(-1))
    assert (u16(zh)[n:] == NAN16).all() and (u16(zl)[n:] == NAN16).all()


# ---------------------------------------------------------------- above the clamp
def test_above_the_clamp(ops):
    """The whole ladder, 65519.99, 65520, +-1e9 and the random values up to 2^17 included: every producer clamps BEFORE it takes the
    lo half (bits still equal the restatement's) and raises the saturation flag."""
    n = LADDER.size // 32 * 32
    xs = np.concatenate((LADDER[:sr.SPECIALS.size], LADDER[-(n - sr.SPECIALS.size):]))
    assert (np.abs(xs) > 65504.0).sum() > 8
    x = torch.from_numpy(xs).to(DEV)
    want_hi, want_lo = sr.split_pair(xs)

    def flagged(fn):
        ops.saturation_reset()
        fn()
        v = ops.saturation_query()
        ops.saturation_reset()
        return v
    hi, lo = f16_buffer(n), f16_buffer(n)
    assert flagged(lambda: ops.split_act_f16(x, hi, lo)) != 0
    assert np.array_equal(u16(hi), u16(want_hi)) and np.array_equal(u16(lo), u16(want_lo))
    il = ops.SplitIL(n // 32, 32, DEV)
    assert flagged(lambda: ops.split_act_f16(x.view(n // 32, 32), il)) != 0
    assert np.array_equal(u16(il.buf), u16(sr.interleave(want_hi.reshape(-1, 32), want_lo.reshape(-1, 32))))
    zh, zl = f16_buffer(n), f16_buffer(n)
    assert flagged(lambda: ops.hifigan_split_channels_last(x.view(1, n // 4, 4), (zh.view(1, n // 4, 4), zl.view(1, n // 4, 4)), 0.1)) != 0
    a_hi, a_lo = sr.split_pair(np.where(xs > 0, xs, xs * np.float32(0.1)).astype(np.float32))
    assert np.array_equal(u16(zh), u16(a_hi)) and np.array_equal(u16(zl), u16(a_lo))
    W = xs[:32 * 8].reshape(8, 32)
    out = f16_buffer(8 * 64)
    assert flagged(lambda: ops.split_f16_colscale_il(torch.from_numpy(W).to(DEV), torch.ones(1, 32, device=DEV), None, 1.0, out.view(1, 8, 64))) != 0
    assert np.array_equal(u16(out).reshape(1, 8, 64), u16(sr.colscale_il(W, np.ones((1, 32), np.float32), None, 1.0)))


# ---------------------------------------------------------------- layouts the kernels cannot address are refused
def _ceil32(n):
    return (n + 31) // 32 * 32


def test_split_f16_dev_refuses_interleaved_partial_block(ops):
    """lo == hi + 32 with n % 32 != 0: element 39's lo half would sit at index 103 of a pair that ends at 80.  The buffer is large
    enough for that store anyway: this test can never write out of bounds, whatever the library does."""
    from covomix_amd import _lib
    n = 40
    buf = f16_buffer(2 * _ceil32(n) + 64)
    x = torch.zeros(n, device=DEV)
    ops.ensure_saturation_bound()
    with pytest.raises(_lib.CovomixHipError, match="n % 32"):
        _lib.check(_lib.load().cvx_split_f16_dev(x.data_ptr(), buf.data_ptr(), buf.data_ptr() + 64, n, 1.0, None, ops._stream()), "cvx_split_f16_dev")
    torch.cuda.synchronize()
    assert (u16(buf) == NAN16).all()
    # a multiple of 32 is taken, through the same call
    _lib.check(_lib.load().cvx_split_f16_dev(x.data_ptr(), buf.data_ptr(), buf.data_ptr() + 64, 32, 1.0, None, ops._stream()), "cvx_split_f16_dev")
    assert (u16(buf)[:64] == 0).all() and (u16(buf)[64:] == NAN16).all()


def test_adarmsnorm_refuses_interleaved_rows_that_are_no_multiple_of_32(ops):
    """y_lo == y_hi + 32 with D % 32 != 0: the flat-offset layout map would scatter a row over its neighbours' lines.  Buffer sized so
    that even those stores would stay inside it."""
    from covomix_amd import _lib
    rows, D = 3, 40
    buf = f16_buffer(2 * rows * D + 64)
    x, g = torch.ones(rows, D, device=DEV), torch.ones(D, device=DEV)
    ops.ensure_saturation_bound()

    def call(d):
        return _lib.load().cvx_adarmsnorm_scaled_f32(x.data_ptr(), g.data_ptr(), None, None, buf.data_ptr(), buf.data_ptr() + 64, rows, d, rows,
                                                     float(d) ** 0.5, 1e-12, None, ops._stream())
    with pytest.raises(_lib.CovomixHipError, match="D % 32"):
        _lib.check(call(D), "cvx_adarmsnorm_scaled_f32")
    torch.cuda.synchronize()
    assert (u16(buf) == NAN16).all()
    _lib.check(call(32), "cvx_adarmsnorm_scaled_f32")          # (reads x as [3, 32]: rows of ones -> hi = 1, lo = 0)
    got = u16(buf)
    assert (got[:2 * rows * 32].reshape(rows, 2, 32)[:, 0] == 0x3C00).all() and (got[:2 * rows * 32].reshape(rows, 2, 32)[:, 1] == 0).all()
    assert (got[2 * rows * 32:] == NAN16).all()


def test_front_ends_refuse_a_padded_splitil(ops):
    """Neither cvx_split_f16_dev nor cvx_adarmsnorm_scaled_f32 takes a row stride: a SplitIL whose rows are views into a wider buffer
    is refused on the host, before any launch."""
    rows, cols = 4, 32
    wide = ops.SplitIL(rows, 2 * cols, DEV)
    view = wide.rows_view(0, rows)
    view.cols = cols                                           # rows of 2 * cols halves inside lines of 4 * cols
    assert view.buf.stride(0) == 4 * cols
    wide.buf.view(torch.int16).fill_(NAN16)
    x = torch.ones(rows, cols, device=DEV)
    with pytest.raises(AssertionError):
        ops.split_act_f16(x, view)
    with pytest.raises(AssertionError):
        ops.adarmsnorm(x, torch.ones(cols, device=DEV), None, None, out_split=view)
    with pytest.raises(AssertionError):
        ops.adarmsnorm(x, torch.ones(cols, device=DEV), None, torch.empty_like(x), out_split=view)
    torch.cuda.synchronize()
    assert (u16(wide.buf) == NAN16).all()
