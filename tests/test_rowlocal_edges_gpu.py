"""The small row-local kernels at the shapes where each of their code paths begins or ends, against a plain fp64 reference of the
same operation: cvx_rownorm_scale_f32, cvx_geglu_f32, cvx_gemm_skinny_f32 (padded strides, a second trip of the tile loop, the
tanh epilogue, two K chunks and a tail), cvx_amax_pow2_scale_f32 / cvx_pow2_scale_from_amax_f32 (where the maximum sits),
cvx_dwconv31_gelu_res_f32 (dense), cvx_embed_gather_f32, cvx_time_fourier_f32, cvx_wav_to_int16.

Per-element bounds next to a rel_l2 (geglu, dwconv) are not invented: the same formula is evaluated in plain fp32 with torch on the
CPU on the same inputs, its largest deviation from fp64 relative to |ref| + max|ref| is taken over the cases of the test, and the
kernel is allowed four times that (it differs from the fp32 evaluation in summation order and in a 1-ulp erf, not in the algorithm)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_restated as sr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 2e-6          # rel_l2 of tests/test_kernels_gpu.py: fp32 products, differences are summation order only


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import covomix_amd.ops as o
    return o


def randn(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed))


def deviation(got, ref):
    """max |got - ref| / (|ref| + max|ref|)"""
    got, ref = got.double().cpu(), ref.double().cpu()
    return float(((got - ref).abs() / (ref.abs() + ref.abs().max())).max())


# ---------------------------------------------------------------- cvx_rownorm_scale_f32
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("parts,ld", [(1, 1), (1, 4), (3, 3), (3, 4), (4, 4), (4, 5), (4, 8), (16, 16), (16, 17), (16, 20),
                                      (64, 64), (64, 65), (64, 68)])
def test_rownorm_scale(ops, parts, ld, rows):
    """ld == parts and padded; parts % 4 == 0 with an odd ld must take the scalar loop (a 16-byte load would be misaligned), with
    ld % 4 == 0 the 16-byte loop; one block and a second block of one row; an all-zero row gives scale / eps."""
    scale, eps = float(parts * 64) ** 0.5, 1e-12
    q = torch.rand(rows, ld, generator=torch.Generator().manual_seed(parts * 100 + ld)) * 50.0
    q[:, parts:] = float("nan")                              # the padding is never read
    zero = 100 if rows > 100 else None
    if zero is not None:
        q[zero, :parts] = 0.0
    out = torch.full((rows + 1,), float("nan"), device=DEV)
    ops.rownorm_scale(q.to(DEV), rows, parts, out, scale, eps)
    got = out.cpu().double()
    assert torch.isnan(got[rows])                             # nothing behind the last row
    s32, e32 = float(np.float32(scale)), float(np.float32(eps))
    ref = s32 / torch.clamp_min(q[:, :parts].double().sum(dim=1).sqrt(), e32)
    # a sum of `parts` non-negative terms in index order is off by at most (parts - 1) roundings of 2^-24 each (relative); the square
    # root halves that and rounds once, the maximum not at all, the quotient once - 2^-24 each if correctly rounded, twice that for
    # a 1-ulp square root and quotient: ((parts - 1) / 2 + 4) * 2^-24.  The all-zero row (scale / eps) is held to the same bound.
    bound = ((parts - 1) / 2 + 4) * 2.0 ** -24
    rel = (got[:rows] - ref).abs() / ref
    assert float(rel.max()) <= bound, (float(rel.max()), bound)
    if zero is not None:
        assert float(ref[zero]) == s32 / e32 and float(rel[zero]) <= bound


def test_rownorm_scale_rejects(ops):
    from covomix_amd import _lib
    out = torch.empty(8, device=DEV)
    with pytest.raises(_lib.CovomixHipError):
        ops.rownorm_scale(torch.ones(8, 65, device=DEV), 8, 65, out, 1.0)                       # more than 64 parts
    off = torch.ones(8 * 8 + 1, device=DEV)[1:].view(8, 8)                                        # base 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    with pytest.raises(_lib.CovomixHipError):
        ops.rownorm_scale(off, 8, 4, out, 1.0)                                                     # parts % 4 == 0, ld % 4 == 0: the 16-byte loop
    ops.rownorm_scale(off, 8, 3, out, 2.0)                                                         # the scalar loop takes the same view
    assert torch.allclose(out.cpu(), torch.full((8,), 2.0 / 3.0 ** 0.5), rtol=1e-6)


# ---------------------------------------------------------------- cvx_geglu_f32
GEGLU_CASES = [(1, 3, 3), (5, 130, 136), (3, 683, 704)]


def _geglu_inputs(rows, Fd):
    return randn(rows, 2 * Fd, seed=rows * 1000 + Fd)


@pytest.fixture(scope="module")
def geglu_fp32_deviation():
    d = 0.0
    for rows, Fd, _ in GEGLU_CASES:
        h = _geglu_inputs(rows, Fd)
        d = max(d, deviation(h[:, :Fd] * F.gelu(h[:, Fd:]), h[:, :Fd].double() * F.gelu(h[:, Fd:].double())))
    return d


@pytest.mark.parametrize("rows,Fd,ld_out", GEGLU_CASES)
def test_geglu(ops, geglu_fp32_deviation, rows, Fd, ld_out):
    """No padding at all, eight padding columns with rows * ld_out below three blocks, and a wide pad: columns below F against fp64,
    columns F..ld_out exactly zero (out is prefilled with NaN)."""
    h = _geglu_inputs(rows, Fd)
    out = torch.full((rows, ld_out), float("nan"), device=DEV)
    ops.geglu(h.to(DEV), out, Fd)
    got = out.cpu()
    ref = h[:, :Fd].double() * F.gelu(h[:, Fd:].double())
    assert rel_l2(got[:, :Fd], ref) < TOL
    # plain fp32 on the CPU deviates from fp64 by 5.8e-08 (relative to |ref| + max|ref|, largest over the three cases): bound 2.3e-07
    d = deviation(got[:, :Fd], ref)
    print(f"geglu rows={rows} F={Fd}: deviation {d:.3e}, fp32 on the CPU {geglu_fp32_deviation:.3e}")
    assert d <= 4 * geglu_fp32_deviation, (d, geglu_fp32_deviation)
    assert (got[:, Fd:] == 0).all()


# ---------------------------------------------------------------- cvx_gemm_skinny_f32
def _skinny(ops, M, N, K, act, bias, pads=(4, 8, 1), seed=0):
    """a, w, out as column slices of wider tensors (lda > K, ldw > K, ldc > N); out's padding columns hold NaN.  -> (out slice, wide out, ref)"""
    pa, pw, po = pads
    a_w, w_w = randn(M, K + 2 * pa, seed=seed + 1), randn(N, K + 2 * pw, seed=seed + 2) / math.sqrt(K)
    b = randn(N, seed=seed + 3) if bias else None
    ad, wd = a_w.to(DEV), w_w.to(DEV)
    o_w = torch.full((M, N + 2 * po + 1), float("nan"), device=DEV)
    a, w, out = ad[:, pa:pa + K], wd[:, pw:pw + K], o_w[:, po:po + N]
    assert a.stride(0) > K and w.stride(0) > K and out.stride(0) > N
    ops.gemm_skinny(a, w, out, bias=b.to(DEV) if bias else None, act=act)
    ref = a_w[:, pa:pa + K].double() @ w_w[:, pw:pw + K].double().t()
    if bias:
        ref = ref + b.double()
    ref = [ref, F.gelu(ref), F.silu(ref), torch.tanh(ref)][act]
    return out, o_w, ref, po


def _tile_errors(got, ref):
    """rel_l2 per tile of 32 columns (one wave's tile): one bad tile cannot be averaged away."""
    got, ref = got.double().cpu(), ref.double()
    N = ref.shape[1]
    worst = 0.0
    for n0 in range(0, N, 32):
        worst = max(worst, float((got[:, n0:n0 + 32] - ref[:, n0:n0 + 32]).norm() / ref[:, n0:n0 + 32].norm().clamp_min(1e-30)))
    return worst


@pytest.mark.parametrize("M,N,K,act,bias", [(7, 333, 264, 0, True),        # padded strides, K with an 8-column tail of a 16-step round
                                            (5, 100, 64, 3, False),       # tanh, no bias
                                            (32, 130, 2056, 3, True),     # two full 1024-column chunks of A in LDS and an 8-column tail
                                            (1, 33, 1032, 1, False)])     # one row, a chunk and a tail
def test_gemm_skinny_padded_strides(ops, M, N, K, act, bias):
    out, o_w, ref, po = _skinny(ops, M, N, K, act, bias, seed=M + N + K)
    assert rel_l2(out, ref) < TOL
    assert _tile_errors(out, ref) < TOL
    assert torch.isnan(o_w[:, :po]).all() and torch.isnan(o_w[:, po + N:]).all()           # the padding columns survive


def test_gemm_skinny_second_trip(ops):
    """M = 32, N = 256 * 128 + 160, K = 64: ceil(N / 128) = 258 groups of four tiles on min(258, CUs) blocks - with 256 CUs block 0
    walks a second trip with all four waves busy (tiles 1024..1027) and block 1 one in which only wave 0 holds a tile (1028, the
    last of ceil(N / 32) = 1029); with fewer CUs more blocks do."""
    M, N, K = 32, 256 * 128 + 160, 64
    assert (N + 127) // 128 > ops.stream_cus() and (N + 31) // 32 % 4 != 0
    out, o_w, ref, po = _skinny(ops, M, N, K, 0, True, seed=9)
    assert rel_l2(out, ref) < TOL
    assert _tile_errors(out, ref) < TOL
    assert torch.isnan(o_w[:, :po]).all() and torch.isnan(o_w[:, po + N:]).all()


def test_gemm_skinny_empty_problems_touch_nothing(ops):
    """M = 0 and N = 0 return before any launch (through the C ABI: an empty torch tensor has no address to pass)."""
    from covomix_amd import _lib
    a, w = torch.ones(4, 64, device=DEV), torch.ones(8, 64, device=DEV)
    out = torch.full((4, 8), float("nan"), device=DEV)
    for M, N in ((0, 8), (4, 0), (0, 0)):
        _lib.check(_lib.load().cvx_gemm_skinny_f32(a.data_ptr(), 64, w.data_ptr(), 64, None, out.data_ptr(), 8, M, N, 64, 0, ops._stream()),
                   "cvx_gemm_skinny_f32")
    assert torch.isnan(out).all()
    ops.gemm_skinny(a, w, out)
    assert torch.equal(out.cpu(), torch.full((4, 8), 64.0))


# ---------------------------------------------------------------- cvx_amax_pow2_scale_f32 / cvx_pow2_scale_from_amax_f32
def _amax_plants(n):
    """Element indices at which a lone maximum must be found, from amax_kernel's own launch arithmetic:
         n4     = n // 4 groups of four floats, the n % 4 elements behind them are read one by one by block 0
         blocks = ceil(n4 / 1024) + 1, at most 2048;   stride = 256 * blocks threads
         thread t reads groups t, t + stride, ... : FOUR per trip while t + 4 * stride * m + 3 * stride < n4 (the unrolled loop,
         q(t) = ceil(max(0, n4 - t - 3 * stride) / (4 * stride)) trips), then one per trip (the remainder loop).
       So group j (thread j % stride, its read number j // stride) is an unrolled read iff j // stride < 4 * q(j % stride)."""
    n4 = n // 4
    g = (n4 + 1023) // 1024
    blocks = g + 1 if g < 2048 else 2048
    stride = 256 * blocks
    plants = {"first": 0, "last": n - 1}
    if n4 > 0:
        j = np.arange(n4, dtype=np.int64)
        t, k = j % stride, j // stride
        q = np.maximum(0, -(-(n4 - t - 3 * stride) // (4 * stride)))
        unrolled = k < 4 * q
        if unrolled.any():
            plants["unrolled"] = int(4 * j[unrolled][-1] + 2)          # the last unrolled group, third float
        if (~unrolled).any():
            plants["remainder"] = int(4 * j[~unrolled][-1] + 1)        # the last group only the remainder loop reaches
    return plants, blocks, stride


def test_amax_plants_arithmetic():
    """(host arithmetic only) the sizes below reach what they are meant to."""
    p, blocks, stride = _amax_plants(65536 + 3)                        # n4 = 16384 -> 17 blocks, stride 4352: threads below 3328 unroll once
    assert (blocks, stride) == (17, 4352) and "unrolled" in p and "remainder" in p
    p, blocks, stride = _amax_plants(4099)                             # n4 = 1024 -> 2 blocks, stride 512: 512 + 3 * 512 >= 1024, no unrolled trip
    assert (blocks, stride) == (2, 512) and "unrolled" not in p and p["remainder"] == 4 * 1023 + 1
    p, blocks, stride = _amax_plants(2048 * 1024 * 4 * 2 + 1)          # n4 = 8 * stride: two unrolled trips per thread, no remainder
    assert (blocks, stride) == (2048, 524288) and p["unrolled"] == 4 * (2048 * 1024 * 2 - 1) + 2 and "remainder" not in p
    assert _amax_plants(2048 * 1024 * 4 * 2 - 3)[0].get("remainder") is not None      # one group fewer: some threads take one trip only
    assert set(_amax_plants(3)[0]) == {"first", "last"}


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099, 65536 + 3, 2048 * 1024 * 4 * 2 + 1])
def test_amax_pow2_scale_finds_a_lone_maximum(ops, n):
    """Zeros with one +-1.3 * 2^k planted at the first element, the last (a one-by-one tail element when n % 4 != 0), in the four-deep
    unrolled loop and where only the remainder loop reads.  The last n is the smallest at which threads take a second trip on the
    capped grid of 2048 blocks (64 MiB, one pass each).  1.3 keeps log2(target / amax) at a fraction of about 0.62: a log2f that is an
    ulp off cannot move the rounded exponent."""
    plants, _, _ = _amax_plants(n)
    x = torch.zeros(n, device=DEV)
    scale = torch.full((1,), float("nan"), device=DEV)
    scratch = torch.zeros(1, dtype=torch.int32, device=DEV)
    target = 1024.0
    ops.amax_pow2_scale(x, target, scale, scratch)
    assert float(scale) == 1.0 and int(scratch) == 0                   # all zeros
    for i, (where, idx) in enumerate(sorted(plants.items())):
        k = (-7, 5, 11, -2)[i]
        v = (1.3 * 2.0 ** k) * (-1.0 if i % 2 else 1.0)
        x[idx] = v
        scale.fill_(float("nan"))
        ops.amax_pow2_scale(x, target, scale, scratch)
        want = sr.pow2_scale(abs(v), target)
        assert float(scale) == float(want), (where, idx, float(scale), float(want))
        assert int(scratch) == 0, where                                 # the scratch word is left zero
        x[idx] = 0.0


def test_pow2_scale_from_amax_clamps(ops):
    scale = torch.empty(1, device=DEV)
    for amax, want in ((1e-30, 2.0 ** 40), (3e38, 2.0 ** -40), (0.0, 1.0), (1.3 * 2.0 ** 3, 2.0 ** 7)):
        assert float(sr.pow2_scale(amax, 1024.0)) == want
        bits = torch.tensor([amax], dtype=torch.float32).view(torch.int32).to(DEV)
        ops.pow2_scale_from_amax(bits, 1024.0, scale)
        assert float(scale) == want and int(bits) == 0
    x = torch.zeros(12, device=DEV)
    scratch = torch.zeros(1, dtype=torch.int32, device=DEV)
    for amax, want in ((1e-30, 2.0 ** 40), (3e38, 2.0 ** -40)):
        x[7] = -amax
        ops.amax_pow2_scale(x, 1024.0, scale, scratch)
        assert float(scale) == want and int(scratch) == 0


# ---------------------------------------------------------------- cvx_dwconv31_gelu_res_f32, dense
DWCONV_CASES = [(1, 1, 4), (2, 15, 80), (1, 16, 260), (3, 17, 64), (1, 47, 300)]


def _dwconv_inputs(Bt, T, C):
    s = Bt * 10000 + T * 100 + C
    return randn(Bt, T, C, seed=s), randn(C, 31, seed=s + 1) / 5, randn(C, seed=s + 2)


def _dwconv_formula(x, w, b):
    C = x.shape[-1]
    return F.gelu(F.conv1d(x.transpose(1, 2), w[:, None, :], b, padding=15, groups=C)).transpose(1, 2) + x


@pytest.fixture(scope="module")
def dwconv_fp32_deviation():
    d = 0.0
    for case in DWCONV_CASES:
        x, w, b = _dwconv_inputs(*case)
        d = max(d, deviation(_dwconv_formula(x, w, b), _dwconv_formula(x.double(), w.double(), b.double())))
    return d


@pytest.mark.parametrize("Bt,T,C", DWCONV_CASES)
def test_dwconv31_dense_edges(ops, dwconv_fp32_deviation, Bt, T, C):
    """T below, at and one past the 16-frame tile (and a single frame), C neither a multiple of 64 nor of 256 (a partly filled
    wave, a second block of four channels), several sequences: every window is cut by a sequence end."""
    x, w, b = _dwconv_inputs(Bt, T, C)
    y = torch.full((Bt, T, C), float("nan"), device=DEV)
    ops.dwconv31_gelu_res(x.to(DEV), w.to(DEV), b.to(DEV), y, Bt, T)
    ref = _dwconv_formula(x.double(), w.double(), b.double())
    assert rel_l2(y, ref) < TOL
    # plain fp32 on the CPU deviates from fp64 by 1.3e-07 (relative to |ref| + max|ref|, largest over the five cases): bound 5.3e-07
    d = deviation(y, ref)
    print(f"dwconv Bt={Bt} T={T} C={C}: deviation {d:.3e}, fp32 on the CPU {dwconv_fp32_deviation:.3e}")
    assert d <= 4 * dwconv_fp32_deviation, (d, dwconv_fp32_deviation)


def test_dwconv31_rejects_in_place(ops):
    from covomix_amd import _lib
    x, w, b = (t.to(DEV) for t in _dwconv_inputs(1, 16, 8))
    with pytest.raises(_lib.CovomixHipError):
        ops.dwconv31_gelu_res(x, w, b, x, 1, 16)


# ---------------------------------------------------------------- the small ones
def test_gather_clamps_fourier_odd_half_int16_wraps(ops):
    # embed_gather: ids below 0 and at / above the table's row count clamp to the first and the last row
    M, S, E, Cc, rows_t = 6, 2, 20, 12, 9
    table, cond = randn(rows_t, E, seed=1), randn(M, Cc, seed=2)
    ids = torch.tensor([[0, 8], [-1, 9], [-2 ** 40, 2 ** 40], [3, -5], [8, 10 ** 6], [4, 4]], dtype=torch.int64)
    out = torch.full((M, S * E + Cc), float("nan"), device=DEV)
    ops.embed_gather(ids.to(DEV), S, table.to(DEV), cond.to(DEV), None, Cc, rows_t - 1, out, M)
    want = torch.cat((table[ids.clamp(0, rows_t - 1)].reshape(M, S * E), cond), dim=-1)
    assert torch.equal(out.cpu(), want)
    # time_fourier: half = 300 is no multiple of the block's 256 threads.  The kernel takes the angle ((t * w) * 2) * pi in fp32 (the
    # reference below takes the same three products) and sinf / cosf of it: at most 4 ulp of a value below 1 (OpenCL's bound), 4.8e-7
    half = 300
    t, wf = torch.tensor([0.0, 0.03125, 0.7, 1.0]), randn(half, seed=3)
    f = torch.full((4, 2 * half), float("nan"), device=DEV)
    ops.time_fourier(t.to(DEV), wf.to(DEV), f)
    ang = ((t.numpy()[:, None] * wf.numpy()[None, :]).astype(np.float32) * np.float32(2.0) * np.float32(math.pi)).astype(np.float64)
    want = np.concatenate((np.sin(ang), np.cos(ang)), axis=-1)
    assert np.abs(f.cpu().numpy().astype(np.float64) - want).max() <= 5e-7
    # wav_to_int16 over a second block of one element, with products that reach +-32768 and beyond (inside int32): truncation toward
    # zero, then the low 16 bits.  Written out in two casts: numpy's direct float -> int16 cast is platform-dependent out there.
    n = 257
    v = (torch.rand(n, generator=torch.Generator().manual_seed(4)) * 2.4 - 1.2).numpy().astype(np.float32)
    v[:12] = [1.0, -1.0, 1.5, -1.5, 2.0, -2.5, 0.99999, -0.99999, 30000.0, -60000.0, 3.0517578e-05 * 1.5, -3.0517578e-05 * 1.5]
    v[256] = -1.00002
    pcm = ops.wav_to_int16(torch.from_numpy(v).to(DEV))
    want = (v * np.float32(32768.0)).astype(np.int32).astype(np.int16)
    assert pcm.dtype == torch.int16 and np.array_equal(pcm.cpu().numpy(), want)
    assert want[0] == -32768 and want[2] == -16384 and want[4] == 0            # (the cases do wrap)
