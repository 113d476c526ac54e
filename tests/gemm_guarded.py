"""Shared by the GEMM edge suites (test_gemm_p8s_epilogue_edges_gpu.py, test_gemm_medium_edges_gpu.py): NaN-guarded buffers, operand
pairs built on the CPU, the fp64 reference and the fp32 simulation of the split-precision arithmetic, and the medium-problem kernel's
split-K rule restated.

Guard style: every output, and every operand an epilogue or a DMA piece reads, is a view at the top left of a taller, wider buffer
pre-filled with NaN (one guard row, guard columns, row stride > width).  A stray store shows as a finite guard element, a stray load
that reaches a result as a NaN."""
import math

import torch
import torch.nn.functional as F

NAN = float("nan")
F16_MAX = 65504.0
WORKSPACE_FLOATS = 4 * 2048 * 4096        # what ops._splitk_workspace allocates per (device, stream)


def dev():
    return torch.device("cuda:0")


class Guarded:
    """a [rows, cols] view (`.v`) of a NaN-filled [rows + 1, cols + pad] buffer, `shift` columns from its left edge"""

    def __init__(self, rows, cols, dtype=torch.float32, pad=64, data=None, shift=0):
        assert 0 <= shift <= pad
        self.rows, self.cols, self.shift = rows, cols, shift
        self.big = torch.full((rows + 1, cols + pad), NAN, dtype=dtype, device=dev())
        self.v = self.big[:rows, shift:shift + cols]
        if data is not None:
            self.v.copy_(data)

    def guards_untouched(self):
        return (bool(torch.isnan(self.big[:, self.shift + self.cols:]).all()) and bool(torch.isnan(self.big[:, :self.shift]).all())
                and bool(torch.isnan(self.big[self.rows]).all()))

    def unwritten(self):
        return bool(torch.isnan(self.big).all())


def vec(n, data):
    """n elements at the head of a longer NaN-filled vector"""
    big = torch.full((n + 64,), NAN, device=dev())
    big[:n] = data
    return big[:n]


class PairIL(Guarded):
    """an interleaved pair (ops.SplitIL: [hi 32 | lo 32] per 32 columns) whose lines sit inside a wider, taller NaN-filled buffer"""

    def __init__(self, ops, rows, cols, x=None, scale=1.0, pad=64):
        super().__init__(rows, 2 * cols, torch.float16, pad=pad)
        self.il = ops.SplitIL.__new__(ops.SplitIL)
        self.il.rows, self.il.cols, self.il.buf = rows, cols, self.v
        self.n = cols
        if x is not None:
            xs = (x.float() * scale).contiguous()
            hi = xs.half()
            self.fill(hi, (xs - hi.float()).half())

    def fill(self, hi, lo):
        t = self.v.unflatten(1, (self.n // 32, 2, 32))
        t[:, :, 0] = hi.reshape(self.rows, self.n // 32, 32)
        t[:, :, 1] = lo.reshape(self.rows, self.n // 32, 32)
        return self

    @property
    def pair(self):
        return self.il

    def halves(self):
        t = self.v.unflatten(1, (self.n // 32, 2, 32))
        return t[:, :, 0].reshape(self.rows, self.n), t[:, :, 1].reshape(self.rows, self.n)

    def value(self):
        h, l = self.halves()
        return h.double() + l.double()


class Pair:
    """a (hi, lo) pair of plain fp16 matrices, each inside its own guarded buffer"""

    def __init__(self, rows, cols, pad=64, shift=0):
        self.h, self.l = Guarded(rows, cols, torch.float16, pad=pad, shift=shift), Guarded(rows, cols, torch.float16, pad=pad, shift=shift)
        self.pair = (self.h.v, self.l.v)

    def halves(self):
        return self.h.v, self.l.v

    def value(self):
        return self.h.v.double() + self.l.v.double()

    def guards_untouched(self):
        return self.h.guards_untouched() and self.l.guards_untouched()


# ---- the medium-problem kernel's split-K rule (splitk_factor_p8m in csrc/gemm_f16x3.hip), restated

def splitk_factor_p8m(M, N, K, K1=0):
    """K slices of an interleaved-operand product below 2048 rows when the caller provides the scratch: the most of 8, 4, 2 for which
    the K-tiles divide evenly, a slice keeps 4 K-tiles (eight slices) or 8 K-tiles (four, two), the 128 x 128 tiles times the slices
    stay within 128 blocks (eight slices) or 256, and A | A2 changes over at a slice boundary.  1 = one launch, no reduction."""
    if N % 4:
        return 1
    tiles = len(range(0, M, 128)) * len(range(0, N, 128))
    for slices, most_blocks, least_tiles in ((8, 128, 4), (4, 256, 8), (2, 256, 8)):
        k_tiles, odd = divmod(K, 32 * slices)
        if odd or k_tiles < least_tiles or tiles * slices > most_blocks:
            continue
        if K1 and K1 % (32 * k_tiles):
            continue
        return slices
    return 1


def vt_slot(t):
    """frame -> slot inside a V^T row: frame groups 0, 2, 1, 3 of an aligned block of 16 (vt_slot in csrc/gemm_common.h)"""
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


# ---- operands on the CPU: the same halves the kernels read, an fp64 reference and an fp32 simulation of the kernel's arithmetic

def split_pair(x, scale=1.0):
    """(hi, lo) fp16 halves of x * scale, saturating, as every split store of the library forms them"""
    y = (x.float() * scale).clamp(-F16_MAX, F16_MAX)
    hi = y.half()
    return hi, (y - hi.float()).half()


def split_weight(w):
    """ops.split_f16 on the CPU: (hi, lo, 1 / scale) with the power of two that brings max |w| to [2^13, 2^14)"""
    amax = float(w.abs().max())
    scale = 2.0 ** (13 - math.floor(math.log2(amax)))
    hi, lo = split_pair(w, scale)
    return hi, lo, 1.0 / scale


def pair_value(x32, scale=1.0):
    """what a split store of the fp32 values x32 holds, read back as hi + lo and un-scaled (fp64)"""
    hi, lo = split_pair(x32, scale)
    return (hi.double() + lo.double()) / scale


def act_fn(x, act):
    return F.gelu(x) if act == 1 else F.silu(x) if act == 2 else x


def errors(got, ref):
    """(whole-matrix rel-L2, worst single row's rel-L2) of got against ref, both fp64 on the CPU"""
    got, ref = got.double().cpu(), ref.double().cpu()
    d = got - ref
    return float(d.norm() / ref.norm().clamp_min(1e-30)), float((d.norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max())


class Problem:
    """[A | A2] . W^T: pairs made on the CPU from a seeded generator; `.ref` the fp64 product of the de-quantised pairs, `.sim` the
    three fp32 products of the same halves with the lo x lo term dropped (what the arithmetic alone leaves).  On the GPU every
    operand a DMA piece reads is guarded: A (and A2) are SplitIL views with stride(0) > 2 K, the interleaved W the first N rows of
    an [N + 1, 2 K] buffer whose last row is NaN."""

    def __init__(self, ops, M, N, K, K1=0, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.K1 = M, N, K, K1
        self.g = g
        self.ah, self.al = split_pair(torch.randn(M, K, generator=g))
        self.wh, self.wl, self.inv = split_weight(torch.randn(N, K, generator=g) / math.sqrt(K))
        self.ref = (self.ah.double() + self.al.double()) @ ((self.wh.double() + self.wl.double()) * self.inv).T
        ah, al, wh, wl = self.ah.float(), self.al.float(), self.wh.float(), self.wl.float()
        self.sim = (al @ wh.T + ah @ wl.T + ah @ wh.T) * self.inv
        k1 = K1 if K1 else K
        self.a = PairIL(ops, M, k1).fill(self.ah[:, :k1].to(dev()), self.al[:, :k1].to(dev()))
        self.x = torch.zeros(M, k1, device=dev())                  # (shape and type only: the kernels read the pairs)
        self.w = torch.zeros(N, K, device=dev())
        self.wbig = torch.full((N + 1, 2 * K), NAN, dtype=torch.float16, device=dev())
        t = self.wbig[:N].unflatten(1, (K // 32, 2, 32))
        t[:, :, 0] = self.wh.to(dev()).reshape(N, K // 32, 32)
        t[:, :, 1] = self.wl.to(dev()).reshape(N, K // 32, 32)
        self.kw = dict(w_split=(self.wh.to(dev()), self.wl.to(dev()), self.inv), w_il=(self.wbig[:N], self.inv), a_split=self.a.il)
        self.a2 = None
        if K1:
            self.a2 = PairIL(ops, M, K - K1).fill(self.ah[:, K1:].to(dev()), self.al[:, K1:].to(dev()))
            self.kw.update(a2=torch.zeros(M, K - K1, device=dev()), a2_split=self.a2.il)

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.g)

    def operands_untouched(self):
        return self.a.guards_untouched() and (self.a2 is None or self.a2.guards_untouched()) and bool(torch.isnan(self.wbig[self.N]).all())
