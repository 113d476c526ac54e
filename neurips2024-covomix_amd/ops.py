"""Torch-tensor front ends of the C-ABI kernels.  Tensors are only device memory +
a stream here; every FLOP of the hot path happens in libcovomix_hip.so."""
from __future__ import annotations

import ctypes as C
import os as _os
import functools
import threading
from contextlib import contextmanager
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import ConvArgs, GemmArgs, GemmNorm, GemmSplitIO

ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2


# Launch contexts (include/covomix_hip.h: cvx_ctx): one caller-owned struct per (device, stream) - the stream handle, its sticky
# saturation flag and the CUs it owns.  The library keeps nothing about a stream; everything an entry point needs travels in the
# struct whose ADDRESS is passed where the C prototypes say cvx_stream_t.  Never freed (captured graphs do not hold them, but a
# raw address in flight must stay valid; there are a handful per process).
_CTX: dict = {}


def ctx_of(stream: Optional["torch.cuda.Stream"] = None) -> "_lib.Ctx":
    st = stream if stream is not None else torch.cuda.current_stream()
    key = (st.device.index, st.cuda_stream)
    c = _CTX.get(key)
    if c is None:
        c = _lib.Ctx(st.cuda_stream, None, torch.cuda.get_device_properties(st.device).multi_processor_count, 0)
        _CTX[key] = c
    return c


def _stream() -> int:
    """What the entry points take as `cvx_stream_t`: the address of the current stream's launch context."""
    return C.addressof(ctx_of())


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.CovomixHipError("covomix_amd ops need tensors on the GPU (no CPU fallback exists)")
        if t.dtype != torch.float32:
            raise TypeError(f"expected float32, got {t.dtype}")


class SplitIL:
    """INTERLEAVED split pair of a [rows, cols] fp32 tensor: one fp16 buffer [rows, 2*cols] laid out [hi 32 | lo 32] per
    block of 32 columns, so that a K-step of one row is one 128-byte cache line for the large-problem GEMM's DMA.  The C ABI
    recognises it by lo == hi + 32 halves.  Accepted wherever a (hi, lo) tuple of split ACTIVATIONS is (GEMM A / A2 operands
    and split outputs, norm and attention outputs); only the large-problem kernel (M >= 2048, N >= 512, interleaved weights)
    can consume it."""

    def __init__(self, rows: int, cols: int, device):
        assert cols % 32 == 0
        self.rows, self.cols = rows, cols
        self.buf = torch.empty(rows, 2 * cols, dtype=torch.float16, device=device)

    def rows_view(self, r0: int, r1: int) -> "SplitIL":
        """The same storage restricted to rows [r0, r1) (a contiguous slice: rows are whole interleaved lines)."""
        v = SplitIL.__new__(SplitIL)
        v.rows, v.cols, v.buf = r1 - r0, self.cols, self.buf[r0:r1]
        return v

    def dense(self):
        """(hi, lo) as ordinary [rows, cols] tensors (copies; tests)."""
        b = self.buf.view(self.rows, self.cols // 32, 2, 32)
        return b[:, :, 0].reshape(self.rows, self.cols), b[:, :, 1].reshape(self.rows, self.cols)


def _pair(x, rows=None, cols=None):
    """(hi_ptr, lo_ptr, ld) of a split pair: a (hi, lo) tuple (lo may be None) or a SplitIL."""
    if isinstance(x, SplitIL):
        assert (rows is None or x.rows == rows) and (cols is None or x.cols == cols), "SplitIL shape mismatch"
        assert x.buf.stride(1) == 1 and x.buf.stride(0) >= 2 * x.cols
        return x.buf.data_ptr(), x.buf.data_ptr() + 64, x.buf.stride(0)          # (rows may be padded: a view into a wider buffer)
    hi, lo = x
    assert hi.dtype == torch.float16 and hi.stride(-1) == 1 and hi.is_cuda
    assert (rows is None or hi.shape[0] == rows) and (cols is None or hi.shape[-1] == cols)
    assert lo is None or (lo.dtype == torch.float16 and lo.shape == hi.shape and lo.stride() == hi.stride())
    return hi.data_ptr(), _p(lo), hi.stride(0) if hi.ndim == 2 else hi.shape[-1]


# cvx_gemm_split_io.flags of every interleaved-operand GEMM: 0, the library picks the kernel (for 2048 rows and more by how full the
# large kernel's last round of tiles would be), unless the calling thread pins one with gemm_flags().
_GEMM_FLAGS = 0                  # (the process-wide part, always 0: bench.py reads it to name the GEMM kernel it reports)
_TL = threading.local()          # per-thread additions to the flags (gemm_flags): a schedule that pins a kernel must not leak into other threads


@contextmanager
def gemm_flags(extra: int):
    """with ops.gemm_flags(16): every GEMM THIS THREAD launches inside the block carries the extra cvx_gemm_split_io.flags bits
    (16 = CVX_GEMM_FLAG_NO_MEDIUM pins the large-problem kernel, 64 / 128 its tile height: A/B measurements and the bit-identity
    tests; 512 = CVX_GEMM_FLAG_VT_PIECES keeps to_qkv's earlier 8-byte V^T stores, same bits).  Thread-local: another host thread's solve is not affected (round-4 advice)."""
    old = getattr(_TL, "flags", 0)
    _TL.flags = old | int(extra)
    try:
        yield
    finally:
        _TL.flags = old

_SPLITK_WS: dict = {}
SPLITK_SCRATCH_MAX_ROWS = 2048   # gemm hands the split-K scratch over up to this many rows (acoustic.route names the rule next to its neighbours)


def il_min_rows() -> int:
    """Row count from which GEMM A operands are kept as INTERLEAVED pairs (SplitIL: the medium- and large-problem kernels)."""
    return 128


def _splitk_workspace(device) -> torch.Tensor:
    """Caller-owned scratch of cvx_gemm_f16x3's split-K path: 4 x 2048 x 4096 floats per (device, stream) - two host threads on
    one device run their GEMMs on different streams and must not share partial sums - allocated once and never re-allocated
    (its address is baked into captured HIP graphs; launches inside a capture use the scratch of the stream that captures)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    st = torch.cuda.current_stream(idx)
    key = (idx, _CAPTURE_OWNER.get((idx, st.cuda_stream), st.cuda_stream))
    ws = _SPLITK_WS.get(key)
    if ws is None:
        ws = torch.empty(4 * 2048 * 4096, dtype=torch.float32, device=dev)
        _SPLITK_WS[key] = ws
    return ws


class _CaptureGate:
    """Host threads vs stream capture.  HIP (ROCm 7.2) refuses device-wide synchronisation and synchronous copies from ANY host
    thread while one thread captures a stream: thread-local capture mode does not shield the other threads the way CUDA's does
    (measured: torch.cuda.synchronize() / .item() in thread B fail with hipErrorStreamCaptureUnsupported, thread A's capture
    ends with hipErrorStreamCaptureInvalidated, sometimes the process aborts).  So the package serialises its captures against
    its own entry points: an entry point (model upload, a solve, a vocoder call, a text2semantic decode) holds the gate SHARED
    for its whole host side, a capture (once per shape and stream) holds it EXCLUSIVE.  Steady state - graph replays from many
    threads - is unaffected (shared holders do not exclude each other).  A thread that holds the gate shared and reaches a
    capture gives its share back while it waits, so two such threads cannot deadlock; new shared entries queue behind a
    waiting capture so that it cannot starve.  Torch calls a caller makes from its OWN other threads are outside this gate."""

    def __init__(self):
        self._c = threading.Condition()
        self._readers = 0
        self._writer = False
        self._waiting = 0
        self._tl = threading.local()

    @contextmanager
    def shared(self):
        tl = self._tl
        d = getattr(tl, "depth", 0)
        outer = d == 0 and not getattr(tl, "excl", False)
        if outer:
            with self._c:
                while self._writer or self._waiting:
                    self._c.wait()
                self._readers += 1
        tl.depth = d + 1
        try:
            yield
        finally:
            tl.depth = d
            if outer:
                with self._c:
                    self._readers -= 1
                    self._c.notify_all()

    @contextmanager
    def exclusive(self):
        tl = self._tl
        if getattr(tl, "excl", False):
            yield
            return
        held = getattr(tl, "depth", 0) > 0
        with self._c:
            if held:
                self._readers -= 1
            self._waiting += 1
            self._c.notify_all()
            while self._writer or self._readers > 0:
                self._c.wait()
            self._waiting -= 1
            self._writer = True
        tl.excl = True
        try:
            yield
        finally:
            tl.excl = False
            with self._c:
                self._writer = False
                if held:
                    self._readers += 1
                self._c.notify_all()


CAPTURE_GATE = _CaptureGate()


def gated(fn):
    """Decorator: run the entry point with the capture gate held shared (see _CaptureGate)."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        with CAPTURE_GATE.shared():
            return fn(*args, **kwargs)
    return wrapper


_CAPTURE_OWNER: dict = {}        # (device, side / capture stream) -> the stream whose call it serves (saturation_share)


def _sp(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of an activation pre-scale: a one-element fp32 CUDA tensor (a view into a scale table), or None = 1."""
    if t is None or isinstance(t, int):          # (an int is a raw device address from a pre-computed pointer table)
        return t
    assert t.is_cuda and t.dtype == torch.float32 and t.numel() == 1
    return t.data_ptr()


def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, bias=None, act=ACT_NONE, residual=None,
         a2: Optional[torch.Tensor] = None, rope=None, rope_cols: int = 0, w_split=None,
         a_split=None, a2_split=None, out_split=None, write_f32: bool = True, vt_split=None, w_il=None,
         a_scale=None, c_scale=None, vt_scale=None, norm=None, c_gamma=None, c_rowsq=None, a_row_scale=None,
         res_split=None, res_scale=None, a2_scale=None) -> torch.Tensor:
    """out[M,N] = epilogue([a | a2] @ w[:, :K].T).  `a`, `a2`, `out`, `residual` are 2-D with unit
    inner stride (row stride may exceed the width); `w` may be a column-slice view of a wider matrix.
    w_split = (hi, lo) fp16 halves from split_f16(w): run the split-precision f16x3 MFMA kernel instead
    of the fp32 one (needs K % 32 == 0; small-M problems stay on the fp32 kernel).
    a_split / a2_split = (hi, lo) fp16 copies of a / a2 (then every tile arrives by LDS-DMA; `a` is only used for
    its shape); out_split = (hi, lo) receives a split copy of the result; write_f32=False skips the fp32 store.
    Any `lo` may be None: w_split = (hi, None, 1/scale) selects the single-term fp16 kernel (plain fp16 operands,
    fp32 accumulate; needs a_split and K % 64 == 0), whose inputs / outputs only carry the hi halves.
    a_scale / c_scale / vt_scale: one-element fp32 CUDA tensors (powers of two) - the pre-scale the producer of a_split (and
    a2_split) applied, and the pre-scales to apply to out_split / vt_split (see cvx_gemm_split_io in the header).
    norm = dict(gamma, beta (or None), out_split, scale (device pre-scale or None)[, eps]): the AdaptiveRMSNorm / RMSNorm of the
    rows of `out` as part of the same call (cvx_gemm_f16x3_norm): its split pair feeds the next GEMM; on the split-K path the
    norm rides in the reduction (no launch, no re-read).
    Deferred norm (cvx_gemm_split_io, version 105; interleaved operands only): c_gamma [N] multiplies the columns of out_split,
    c_rowsq [M, >= N/64] receives the rows' sums of squares per 64-column slice (rownorm_scale turns them into one factor per
    row); a_row_scale [M] multiplies the rows of the accumulators of the GEMM that consumes that pair; res_split (+ res_scale) gives
    the residual as a split pair (then residual must be None; may be the very pair out_split names)."""
    _chk_f32(a, w, out, bias, residual, a2)
    M = a.shape[0]
    N = w.shape[0]
    k1 = a.shape[1]
    K = k1 + (a2.shape[1] if a2 is not None else 0)
    assert w.shape[1] == K, f"gemm: K mismatch ({w.shape[1]} vs {K})"
    assert a.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1 and out.shape == (M, N)
    g = GemmArgs()
    g.A, g.lda = a.data_ptr(), a.stride(0)
    if a2 is not None:
        assert a2.shape[0] == M and a2.stride(1) == 1
        g.A2, g.lda2, g.K1 = a2.data_ptr(), a2.stride(0), k1
    else:
        g.A2, g.lda2, g.K1 = None, 0, 0
    g.W, g.ldw = w.data_ptr(), w.stride(0)
    g.C, g.ldc = out.data_ptr(), out.stride(0)
    g.bias = _p(bias)
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1
        g.residual, g.ldr = residual.data_ptr(), residual.stride(0)
    else:
        g.residual, g.ldr = None, 0
    g.M, g.N, g.K, g.act = M, N, K, act
    if rope is not None:
        cos, sin = rope
        _chk_f32(cos, sin)
        g.rope_cos, g.rope_sin, g.rope_T, g.rope_cols = cos.data_ptr(), sin.data_ptr(), cos.shape[0], rope_cols
    else:
        g.rope_cos, g.rope_sin, g.rope_T, g.rope_cols = None, None, 0, 0
    if isinstance(a_split, SplitIL):
        assert w_il is not None, "an interleaved A operand needs interleaved weights"
    # interleaved weights go with an interleaved A: the large- (M >= 2048, N >= 512) and medium-problem kernels
    if w_il is not None and w_split is not None and w_split[1] is not None and isinstance(a_split, SplitIL):
        il, inv_il = w_il                      # interleaved [N, 2K] copy of the same split weight (split_f16_interleaved)
        assert il.dtype == torch.float16 and il.shape == (N, 2 * K) and il.is_contiguous() and il.is_cuda
        use_il = True
    else:
        use_il = False
    if w_split is not None and K % 32 == 0 and (M > 64 or a_split is not None or out_split is not None):
        hi, lo, inv_scale = w_split
        ensure_saturation_bound()
        assert hi.dtype == torch.float16 and hi.shape == (N, K) and hi.stride(1) == 1 and hi.is_cuda
        assert lo is None or (lo.dtype == torch.float16 and lo.shape == (N, K) and lo.stride() == hi.stride() and lo.is_cuda)
        g.ldw = hi.stride(0)                       # rows may be padded (row stride > K)
        io = GemmSplitIO()
        io.write_f32 = 1 if write_f32 else 0
        io.a_scale_dev, io.c_scale_dev, io.vt_scale_dev = _sp(a_scale), _sp(c_scale), _sp(vt_scale)
        if a_split is not None and M <= SPLITK_SCRATCH_MAX_ROWS and rope is None:         # small problems may split K (see the header)
            ws = _splitk_workspace(a.device)
            io.workspace, io.workspace_floats = ws.data_ptr(), ws.numel()
        if a_split is not None:
            io.A_hi, io.A_lo, io.lda_h = _pair(a_split, M, k1)
            if a2 is not None:
                assert a2_split is not None, "pre-split A needs a pre-split A2 as well"
                assert isinstance(a2_split, SplitIL) == isinstance(a_split, SplitIL)
                io.A2_hi, io.A2_lo, io.lda2_h = _pair(a2_split, M, K - k1)
        if out_split is not None:
            io.C_hi, io.C_lo, io.ldc_h = _pair(out_split, M, rope_cols if vt_split is not None else N)
        if a2_scale is not None:
            assert a2 is not None and a_scale is not None
            io.a2_scale_dev = _sp(a2_scale)
        if res_split is not None:
            assert residual is None
            io.R_hi, io.R_lo, io.ldr_h = _pair(res_split, M, N)
            io.r_scale_dev = _sp(res_scale)
        if c_gamma is not None or c_rowsq is not None or a_row_scale is not None:
            _chk_f32(c_gamma, c_rowsq, a_row_scale)
            if c_gamma is not None:
                assert c_gamma.numel() == N and c_gamma.stride(-1) == 1 and out_split is not None
                io.c_gamma_dev = c_gamma.data_ptr()
            if c_rowsq is not None:
                assert c_rowsq.ndim == 2 and c_rowsq.shape[0] >= M and c_rowsq.stride(1) == 1 and c_rowsq.shape[1] * 64 >= N
                io.c_rowsq, io.c_rowsq_ld = c_rowsq.data_ptr(), c_rowsq.stride(0)
            if a_row_scale is not None:
                assert a_row_scale.numel() >= M and a_row_scale.stride(-1) == 1
                io.a_row_scale_dev = a_row_scale.data_ptr()
        if vt_split is not None:          # QKV mode: v columns transposed per (sequence, head) for the f16x3 attention
            vh, vl = vt_split
            assert vh.dtype == torch.float16 and vh.is_contiguous() and (vl is None or (vl.is_contiguous() and vh.shape == vl.shape))
            io.Vt_hi, io.Vt_lo, io.vt_ld = vh.data_ptr(), _p(vl), vh.shape[-1]
        if _lib._DEBUG_SYNC:
            import sys
            print(f"[cvx] gemm_f16x3 M={M} N={N} K={K} k1={g.K1} lo={lo is not None} a_split={a_split is not None} rope={rope is not None} "
                  f"out_split={out_split is not None} vt={vt_split is not None} ws={bool(io.workspace)}", file=sys.stderr, flush=True)
        w_hi_ptr, w_lo_ptr = hi.data_ptr(), _p(lo)
        if use_il:
            io.flags = getattr(_TL, "flags", 0)
            io.w_interleaved, g.ldw = 1, 2 * K
            w_hi_ptr, w_lo_ptr, inv_scale = il.data_ptr(), il.data_ptr() + 64, inv_il
        if norm is not None:
            nm = GemmNorm()
            _chk_f32(norm["gamma"], norm.get("beta"))
            assert norm["gamma"].stride(-1) == 1 and norm["gamma"].numel() == N and out.is_contiguous() and write_f32
            nm.gamma, nm.beta = norm["gamma"].data_ptr(), _p(norm.get("beta"))
            nm.Y_hi, nm.Y_lo, nm.ldy_h = _pair(norm["out_split"], M, N)
            nm.y_scale_dev = _sp(norm.get("scale"))
            nm.scale, nm.eps = float(N) ** 0.5, float(norm.get("eps", 1e-12))
            _lib.check(_lib.load().cvx_gemm_f16x3_norm(C.byref(g), w_hi_ptr, w_lo_ptr, inv_scale, C.byref(io), C.byref(nm), _stream()),
                       "cvx_gemm_f16x3_norm")
            return out
        _lib.check(_lib.load().cvx_gemm_f16x3(C.byref(g), w_hi_ptr, w_lo_ptr, inv_scale, C.byref(io), _stream()),
                   "cvx_gemm_f16x3")
        return out
    assert norm is None, "a fused norm needs the f16x3 kernel"
    assert a_split is None and out_split is None and write_f32, "split I/O needs the f16x3 kernel (w_split, K % 32 == 0, M > 64)"
    assert a_scale is None and c_scale is None and vt_scale is None
    assert c_gamma is None and c_rowsq is None and a_row_scale is None and res_split is None and a2_scale is None, "a deferred norm needs the f16x3 kernel"
    _lib.check(_lib.load().cvx_gemm_bias_act_f32(C.byref(g), _stream()), "cvx_gemm_bias_act_f32")
    return out


GEMM_F32_FORMS = ("T64", "T64_GENERIC", "T128_DMA", "T128_GENERIC")


def gemm_f32_form(M: int, N: int, K: int) -> str:
    """Which kernel the fp32 GEMM (gemm without w_split) launches for this shape, one of GEMM_F32_FORMS: 64- or 128-row tiles,
    register-staged / LDS-DMA operands for K % 32 == 0, predicated loads otherwise.  Host arithmetic of the library's own launch
    rule (cvx_gemm_f32_form): no GPU needed."""
    form = _lib.load().cvx_gemm_f32_form(M, N, K)
    if form < 0:
        raise ValueError(f"gemm_f32_form: no launch has M={M} N={N} K={K}")
    return GEMM_F32_FORMS[form]


def split_act_f16(x: torch.Tensor, hi=None, lo: Optional[torch.Tensor] = None, scale=None):
    """(hi, lo) fp16 halves of an fp32 activation tensor - for GEMMs that take A pre-split.
    With `hi` given and lo=None only the (saturating) fp16 cast is written; hi may be a SplitIL (interleaved pair).
    scale: one-element fp32 CUDA tensor, the power-of-two pre-scale (the consumer GEMM's a_scale); None = 1."""
    _chk_f32(x)
    assert x.is_contiguous()
    ensure_saturation_bound()
    if isinstance(hi, SplitIL):
        h, l, ld = _pair(hi, x.shape[0], x.shape[1])
        assert ld == 2 * hi.cols, "split_act_f16: cvx_split_f16_dev takes no row stride (a SplitIL view into a wider buffer)"
        _lib.check(_lib.load().cvx_split_f16_dev(x.data_ptr(), h, l, x.numel(), 1.0, _sp(scale), _stream()), "cvx_split_f16")
        return hi
    if hi is None:
        hi = torch.empty(x.shape, dtype=torch.float16, device=x.device)
        lo = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _lib.check(_lib.load().cvx_split_f16_dev(x.data_ptr(), hi.data_ptr(), _p(lo), x.numel(), 1.0, _sp(scale), _stream()),
               "cvx_split_f16")
    return hi, lo


def split_f16(w: torch.Tensor, with_lo: bool = True):
    """(hi, lo, 1/scale): fp16 halves of w*scale, hi = fp16(w*scale), lo = fp16(w*scale - hi), with scale the power
    of two that brings max|w| to [2^13, 2^14) so the lo halves stay out of the fp16 subnormal range.
    Load-time weight packing.  with_lo=False: (hi, None, 1/scale) for the single-term fp16 mode."""
    import math
    _chk_f32(w)
    w = w.contiguous()
    amax = float(w.abs().max())
    scale = 2.0 ** (13 - math.floor(math.log2(amax))) if amax > 0 and math.isfinite(amax) else 1.0
    hi = torch.empty(w.shape, dtype=torch.float16, device=w.device)
    lo = torch.empty(w.shape, dtype=torch.float16, device=w.device) if with_lo else None
    ensure_saturation_bound()
    _lib.check(_lib.load().cvx_split_f16(w.data_ptr(), hi.data_ptr(), _p(lo), w.numel(), scale, _stream()),
               "cvx_split_f16")
    return hi, lo, 1.0 / scale


def split_f16_interleaved(w_split):
    """(hi, lo, 1/scale) from split_f16 -> (il [N, 2K], 1/scale) with il[n] = [hi 0:32 | lo 0:32 | hi 32:64 | lo 32:64 | ...]:
    a K-step of one row becomes one 128-byte cache line for the large-problem GEMM's DMA.  Load-time packing."""
    hi, lo, inv = w_split
    N, K = hi.shape
    assert K % 32 == 0 and lo is not None
    il = torch.stack((hi.view(N, K // 32, 32), lo.view(N, K // 32, 32)), dim=2).reshape(N, 2 * K).contiguous()
    return il, inv


def adarmsnorm(x: torch.Tensor, gamma: torch.Tensor, beta: Optional[torch.Tensor], out: Optional[torch.Tensor],
               rows_per_group: Optional[int] = None, eps: float = 1e-12, out_split=None, split_scale=None):
    """out_split = (hi, lo) fp16 tensors: also (or, with out=None, only) write the result as a split pair (times the
    one-element device tensor split_scale, if given)."""
    _chk_f32(x, gamma, beta, out)
    assert x.is_contiguous() and (out is None or out.is_contiguous()) and gamma.stride(-1) == 1
    D = x.shape[-1]
    rows = x.numel() // D
    oh, ol = (None, None)
    if out_split is not None:
        ensure_saturation_bound()
        oh, ol, ld = _pair(out_split, rows if isinstance(out_split, SplitIL) else None, D)
        assert isinstance(out_split, SplitIL) or (out_split[0].is_contiguous() and out_split[0].numel() == x.numel())
        assert not isinstance(out_split, SplitIL) or ld == 2 * D, "adarmsnorm: cvx_adarmsnorm_scaled_f32 takes no row stride (a SplitIL view into a wider buffer)"
    rpg = rows if rows_per_group is None else rows_per_group
    _lib.check(_lib.load().cvx_adarmsnorm_scaled_f32(x.data_ptr(), gamma.data_ptr(), _p(beta), _p(out), oh, ol, rows, D, rpg,
                                                     float(D) ** 0.5, eps, _sp(split_scale), _stream()), "cvx_adarmsnorm_f32")
    return out if out is not None else out_split


def split_f16_colscale_il(w: torch.Tensor, colscale: torch.Tensor, set_scale: Optional[torch.Tensor], scale: float, out: torch.Tensor) -> torch.Tensor:
    """out[s] = interleaved split pair of w * colscale[s][None, :] * set_scale[s] * scale for every set s (cvx_split_f16_colscale_il):
    w [N, K] fp32, colscale [n_sets, K] (row stride free), set_scale [n_sets] (stride free) or None, out [n_sets, N, 2K] fp16."""
    ensure_saturation_bound()
    _chk_f32(w, colscale, set_scale)
    N, K = w.shape
    n_sets = colscale.shape[0]
    assert w.stride(1) == 1 and colscale.shape[1] == K and colscale.stride(1) == 1 and out.dtype == torch.float16 and out.is_contiguous()
    assert tuple(out.shape) == (n_sets, N, 2 * K) and (set_scale is None or set_scale.shape[0] == n_sets)
    _lib.check(_lib.load().cvx_split_f16_colscale_il(w.data_ptr(), w.stride(0), N, K, colscale.data_ptr(), colscale.stride(0), _p(set_scale),
                                                     set_scale.stride(0) if set_scale is not None else 0, n_sets, scale, out.data_ptr(), _stream()),
               "cvx_split_f16_colscale_il")
    return out


def rownorm_scale(rowsq: torch.Tensor, rows: int, parts: int, out: torch.Tensor, scale: float, eps: float = 1e-12) -> torch.Tensor:
    """out[r] = scale / max(sqrt(sum(rowsq[r, :parts])), eps) (cvx_rownorm_scale_f32): the per-row factor of a deferred norm."""
    _chk_f32(rowsq, out)
    assert rowsq.ndim == 2 and rowsq.stride(1) == 1 and rowsq.shape[0] >= rows and rowsq.shape[1] >= parts and out.numel() >= rows and out.stride(-1) == 1
    _lib.check(_lib.load().cvx_rownorm_scale_f32(rowsq.data_ptr(), rows, parts, rowsq.stride(0), scale, eps, out.data_ptr(), _stream()),
               "cvx_rownorm_scale_f32")
    return out


# Saturation flags are CALLER-OWNED: one int32 of device memory per (device, stream), bound to the stream with
# The kernels a stream runs OR bit 0 into the flag of the stream's launch context (two threads / streams on one device never see or
# clear each other's).  Allocated once and never freed (their addresses are baked into captured HIP graphs).
_SAT_FLAGS: dict = {}


def saturation_flag(stream: Optional["torch.cuda.Stream"] = None) -> torch.Tensor:
    """The OWN flag of `stream` (default: the current stream), allocated and put into its launch context on first use.  A flag that
    was only lent to the stream (saturation_share: torch hands stream handles out of a small pool, so a stream a caller just created
    may be the very side / capture stream some earlier call borrowed) is replaced: whoever resets or queries a stream owns its flag."""
    st = stream if stream is not None else torch.cuda.current_stream()
    key = (st.device.index, st.cuda_stream)
    ent = _SAT_FLAGS.get(key)
    if ent is None or ent[1] != key:
        f = torch.zeros(1, dtype=torch.int32, device=st.device)
        torch.cuda.current_stream(st.device).synchronize()        # (the zero fill is on the current stream; `stream` may be another)
        _SAT_FLAGS[key] = (f, key)
        _CAPTURE_OWNER.pop(key, None)
        ctx_of(st).sat_flag = f.data_ptr()
        return f
    return ent[0]


def saturation_share(src: "torch.cuda.Stream", dst: "torch.cuda.Stream") -> None:
    """Kernels launched on `dst` report into the flag of `src` until further notice, and their persistent grids are sized for the
    CUs `src` owns: the capture stream of a HIP graph - and any side stream a call opens - belongs to the call that runs on `src`
    (call it before every such use)."""
    f = saturation_flag(src)
    skey = (src.device.index, src.cuda_stream)
    key = (dst.device.index, dst.cuda_stream)
    if key == skey:
        return
    _CAPTURE_OWNER[key] = src.cuda_stream
    ctx_of(dst).n_cus = ctx_of(src).n_cus
    ent = _SAT_FLAGS.get(key)
    if ent is None or ent[0] is not f:
        _SAT_FLAGS[key] = (f, skey)
        ctx_of(dst).sat_flag = f.data_ptr()


def ensure_saturation_bound() -> None:
    """A call that writes split pairs refuses a launch context without a saturation flag (CVX_EINVAL; a C caller can waive the
    bookkeeping with CVX_CTX_NO_SATURATION_FLAG).  The Python front ends never waive it: every one of them that launches a split-pair
    kernel makes sure the current stream's context has a flag - allocated here on first use outside a capture; inside a capture a
    stream without one is an error (the stream that captures must have been shared with the calling stream: saturation_share)."""
    st = torch.cuda.current_stream()
    if (st.device.index, st.cuda_stream) in _SAT_FLAGS:
        return
    if torch.cuda.is_current_stream_capturing():
        raise _lib.CovomixHipError("a split-precision kernel is being captured on a stream without a saturation flag: call "
                                   "ops.saturation_share(calling_stream, capture_stream) before the capture")
    saturation_flag(st)


# ---------------------------------------------------------------- CU-partitioned streams (include/covomix_hip.h, round 5)
class CUPartition:
    """Two streams of one device on DISJOINT sets of compute units: `main` (the acoustic solve and the vocoder) and `side` (the
    text2semantic decode of the next batch).  Bit k of a HIP CU mask names CU k // 8 of XCD k % 8 and consecutive indices of an XCD go
    round its four shader engines (tools/archive/cu_mask_probe.hip), so `side` takes the top `side_per_xcd` indices of every XCD
    (side_per_xcd a multiple of 4: every shader engine keeps the same number of CUs, which one-block-per-CU kernels need to be
    co-resident - tools/archive/cu_mask_probe2.hip) and `main` the rest.  The streams live as long as the process."""

    def __init__(self, device, side_per_xcd: int = 4):
        dev = torch.device(device)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        n = torch.cuda.get_device_properties(idx).multi_processor_count
        if side_per_xcd <= 0 or side_per_xcd % 4 or n % 8 or 8 * side_per_xcd >= n:
            raise ValueError(f"side_per_xcd must be a positive multiple of 4 below {n // 8} (CUs per XCD), got {side_per_xcd}")
        self.device = torch.device("cuda", idx)
        self.n_side, self.n_main = 8 * side_per_xcd, n - 8 * side_per_xcd
        words = (n + 31) // 32
        lib = _lib.load()

        def make(bits):
            m = (C.c_uint32 * words)()
            for b in bits:
                m[b // 32] |= 1 << (b % 32)
            out = C.c_void_p()
            with torch.cuda.device(idx):
                _lib.check(lib.cvx_stream_create_cu_mask(m, words, C.byref(out)), "cvx_stream_create_cu_mask")
            st = torch.cuda.ExternalStream(out.value, device=self.device)
            ctx_of(st).n_cus = len(bits)               # (what the persistent grids and the GEMM kernel choice are sized from)
            return st
        self.main = make(range(0, self.n_main))
        self.side = make(range(self.n_main, n))


_CU_PARTITIONS: dict = {}


def cu_partition(device=None, side_per_xcd: int = 4) -> CUPartition:
    """The (cached) CUPartition of a device."""
    dev = torch.device(device if device is not None else "cuda")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, side_per_xcd)
    if key not in _CU_PARTITIONS:
        if not _CU_PARTITIONS:
            import atexit
            atexit.register(_destroy_partitions)      # while the HIP runtime is still up (a masked stream that outlives it crashed rocprofv3's finaliser)
        _CU_PARTITIONS[key] = CUPartition(torch.device("cuda", idx), side_per_xcd)
    return _CU_PARTITIONS[key]


def _destroy_partitions() -> None:
    lib = _lib.load()
    for part in list(_CU_PARTITIONS.values()):
        try:
            with torch.cuda.device(part.device):
                torch.cuda.synchronize()
                # torch's pinned-memory allocator keeps events of the streams its blocks were last copied on (the decode's state
                # record travels by non_blocking copies on the side stream): give the blocks back BEFORE their stream goes, or the
                # allocator touches a dead stream at process exit (SIGSEGV, tools/archive/cu_mask_exit_probe.py)
                # (without that call the streams are left to process teardown: destroying them under live pinned blocks is the crash)
                if hasattr(torch._C, "_host_emptyCache"):
                    torch._C._host_emptyCache()
                    for st in (part.main, part.side):
                        st.synchronize()
                        _CTX.pop((st.device.index, st.cuda_stream), None)
                        _SAT_FLAGS.pop((st.device.index, st.cuda_stream), None)
                        lib.cvx_stream_destroy(st.cuda_stream)
        except Exception:               # noqa: BLE001 - interpreter shutdown: nothing left to report to
            pass
    _CU_PARTITIONS.clear()


def is_partition_stream(stream: Optional["torch.cuda.Stream"] = None) -> bool:
    """Is `stream` (default: the current one) one of the CU-masked streams of a CUPartition?"""
    st = stream if stream is not None else torch.cuda.current_stream()
    return any(st.cuda_stream in (p.main.cuda_stream, p.side.cuda_stream) for p in _CU_PARTITIONS.values())


def stream_cus(stream: Optional["torch.cuda.Stream"] = None) -> int:
    """CUs the library sizes persistent grids for on `stream` (default: the current stream)."""
    st = stream if stream is not None else torch.cuda.current_stream()
    n = ctx_of(st).n_cus
    return int(n) if n > 0 else torch.cuda.get_device_properties(st.device).multi_processor_count


def clock_stamps() -> torch.Tensor:
    """[2048, 2] int64 (enqueued on the current stream): per (XCD, CU) slot that CU's shader-clock cycle counter and the 100 MHz real-time
    counter (zero where no block landed).  Pair two calls slot by slot with clock_from_stamps."""
    out = torch.zeros(2048, 2, dtype=torch.int64, device=torch.cuda.current_device())
    _lib.check(_lib.load().cvx_clock_stamps(out.data_ptr(), _stream()), "cvx_clock_stamps")
    return out


def clock_from_stamps(c0: torch.Tensor, c1: torch.Tensor) -> dict:
    """Shader clock of the (busy) region between two clock_stamps() calls: cycles counted / real time on every CU that holds both stamps,
    averaged per XCD -> {mhz (mean over XCDs), xcd_mhz (8 values), cus (CUs paired)}; {} when nothing could be paired."""
    a, b = c0.cpu(), c1.cpu()
    ok = (a[:, 1] != 0) & (b[:, 1] != 0)
    d = (b - a).double()
    ok &= (d[:, 1] > 0) & (d[:, 0] > 0)
    if not bool(ok.any()):
        return {}
    mhz = torch.where(ok, d[:, 0] / d[:, 1].clamp_min(1.0) * 100.0, torch.zeros_like(d[:, 0])).view(8, 256)      # the real-time counter: 100 MHz
    n = ok.view(8, 256).sum(dim=1)
    per_xcd = [float(mhz[x].sum() / n[x]) for x in range(8) if int(n[x]) > 0]
    return {"mhz": sum(per_xcd) / len(per_xcd), "xcd_mhz": per_xcd, "cus": int(ok.sum())}


def saturation_reset() -> None:
    """Clear the current stream's sticky saturation flag (enqueued on that stream; no host synchronisation)."""
    saturation_flag()
    _lib.check(_lib.load().cvx_saturation_flag_reset(_stream()), "cvx_saturation_flag_reset")


def saturation_query(reset: bool = True) -> int:
    """The current stream's sticky saturation flag after everything enqueued so far on it (synchronises that stream):
    non-zero = some split-pair store since the last reset had to clamp (or a softmax normaliser was not finite) - the
    split-precision result must not be trusted."""
    saturation_flag()
    v = C.c_uint32(0)
    _lib.check(_lib.load().cvx_saturation_flag_query(C.byref(v), 1 if reset else 0, _stream()), "cvx_saturation_flag_query")
    return int(v.value)


_SAT_DEFER = threading.local()


def saturation_checked() -> bool:
    """Do the entry points check the saturation flag themselves (reset before, blocking read after)?  False under
    CVX_SAT_CHECK=0 and inside `saturation_deferred()`."""
    return _os.environ.get("CVX_SAT_CHECK", "1") == "1" and getattr(_SAT_DEFER, "depth", 0) == 0


class saturation_deferred:
    """with ops.saturation_deferred() as guard: ...several entry-point calls on the current stream...
    ONE reset before and ONE flag read after the whole block instead of a blocking read per call (round-3 advice: the per-call
    reads are host synchronisations between acoustic model and vocoder, and they keep the entry points out of a caller's own
    stream capture).  Inside the block the entry points return their split-precision results unchecked; afterwards
    `guard.flagged` says whether ANY of them saturated - the caller must then discard the block's results and repeat the calls
    outside the block (where each call checks itself and a flagged one re-runs in fp32 or raises).  `read=False`: no read at
    exit either (a caller that captures the block into its own graph reads the flag with ops.saturation_query() after the
    replay)."""

    def __init__(self, read: bool = True):
        self.read, self.flagged = read, None

    def __enter__(self):
        if getattr(_SAT_DEFER, "depth", 0) == 0 and _os.environ.get("CVX_SAT_CHECK", "1") == "1":
            saturation_reset()
        _SAT_DEFER.depth = getattr(_SAT_DEFER, "depth", 0) + 1
        return self

    def __exit__(self, et, ev, tb):
        _SAT_DEFER.depth -= 1
        if et is None and self.read and _SAT_DEFER.depth == 0 and _os.environ.get("CVX_SAT_CHECK", "1") == "1":
            self.flagged = bool(saturation_query())
        return False


def h2d(t: torch.Tensor, device, dtype=None) -> torch.Tensor:
    """Host tensor -> device through pinned memory, asynchronously on the current stream.  A copy from PAGEABLE memory makes the host
    wait for everything the stream still has to do before it (the runtime stages it behind the queue and waits): one small tensor
    made with torch.tensor(..., device=...) in the middle of a call is enough to keep the host from running ahead of the device."""
    if t.device.type != "cpu":
        return t.to(device=device, dtype=dtype) if dtype is not None else t.to(device)
    if dtype is not None:
        t = t.to(dtype)
    return t.contiguous().pin_memory().to(device, non_blocking=True)


def saturation_snapshot():
    """The current stream's saturation flag as it stands after everything enqueued so far, WITHOUT waiting: an asynchronous copy into a
    pinned int32 tensor (read element 0 once an event recorded after this call has completed).  For callers that run the host ahead
    of the device - `with saturation_deferred(read=False): ...calls...; snap = saturation_snapshot()` - and look at the batch later.
    None under CVX_SAT_CHECK=0."""
    if _os.environ.get("CVX_SAT_CHECK", "1") != "1":
        return None
    snap = torch.zeros(1, dtype=torch.int32).pin_memory()
    snap.copy_(saturation_flag(), non_blocking=True)
    return snap


class Ragged:
    """A packed batch of sequences of different length: sequence i owns rows [cu[i], cu[i+1]) of every [M, width] tensor.
    cu: int32 CUDA tensor [n + 1]; lengths: the python list (host side: grid sizes, slicing)."""

    def __init__(self, lengths, device, repeat: int = 1):
        """repeat = 2: the same sequences twice (conditional rows, then the null-branch rows of CFG)."""
        self.lengths = [int(t) for t in lengths] * repeat
        assert self.lengths and min(self.lengths) > 0
        self.n, self.max_T, self.M = len(self.lengths), max(self.lengths), sum(self.lengths)
        cu = [0]
        for t in self.lengths:
            cu.append(cu[-1] + t)
        self.cu_host = cu
        self.cu_host_i32 = torch.tensor(cu, dtype=torch.int32)      # the host table of the entry points that validate one (adarmsnorm_seq, ...)
        self.cu = h2d(self.cu_host_i32, device)

    def positions(self) -> torch.Tensor:
        """Position of every packed row inside its own sequence (fp32, on the device)."""
        cu = self.cu.to(torch.int64)
        rows = torch.arange(self.M, device=self.cu.device)
        seq = torch.searchsorted(cu[1:], rows, right=True)
        return (rows - cu[seq]).to(torch.float32)


def attention(qkv: torch.Tensor, out: Optional[torch.Tensor], Bt: int, T: int, H: int, scale: float, out_split=None,
              ragged: Optional[Ragged] = None):
    """ragged: packed batch (Bt, T are then ignored: rows = ragged.M, keys restricted to the own sequence)."""
    _chk_f32(qkv, out)
    rows = ragged.M if ragged is not None else Bt * T
    assert qkv.is_contiguous() and (out is None or out.is_contiguous())
    assert qkv.numel() == rows * 3 * H * 64 and (out is None or out.numel() == rows * H * 64)
    oh, ol = (None, None)
    if out_split is not None:
        ensure_saturation_bound()
        oh, ol, _ = _pair(out_split, rows if isinstance(out_split, SplitIL) else None, H * 64)
        assert isinstance(out_split, SplitIL) or (out_split[0].is_contiguous() and out_split[0].numel() == rows * H * 64)
    if ragged is not None:
        _lib.check(_lib.load().cvx_attention_varlen_f32(qkv.data_ptr(), _p(out), oh, ol, ragged.cu.data_ptr(), ragged.n, ragged.max_T,
                                                        H, scale, _stream()), "cvx_attention_varlen_f32")
    else:
        _lib.check(_lib.load().cvx_attention_f32(qkv.data_ptr(), _p(out), oh, ol, Bt, T, H, scale, _stream()),
                   "cvx_attention_f32")
    return out if out is not None else out_split


def vt_frame_slots(T: int, device=None) -> torch.Tensor:
    """Column of frame t in the V^T buffers of the f16x3 attention: bits 2 and 3 of t swapped (four-frame groups in the
    order 0, 2, 1, 3 inside every 16 frames) - what the to_qkv epilogue writes and the attention kernel reads."""
    t = torch.arange(T, device=device)
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def attention_f16x3(qk_split, vt_split, out: Optional[torch.Tensor], Bt: int, T: int, H: int, scale: float, out_split=None,
                    qk_scale=None, v_scale=None, out_scale=None, ragged: Optional[Ragged] = None):
    """Split-precision attention on the pairs written by gemm(..., out_split=qk_split, vt_split=vt_split).
    (hi, None) pairs select the single-term fp16 kernel.  qk_scale / v_scale: the pre-scales the producer applied to the
    pairs (c_scale / vt_scale of the to_qkv GEMM); out_scale: pre-scale of out_split (a_scale of the to_out GEMM).
    ragged: packed batch - qk pairs [M, 2*H*64], vt pairs [H*64, >= M rounded up to 32] written by a to_qkv GEMM that ran
    with per-row RoPE tables [M, 32] (rope_T = M); Bt, T are ignored."""
    qh, ql = qk_split
    vh, vl = vt_split
    ensure_saturation_bound()
    assert (ql is None) == (vl is None)
    for t in (qh, ql, vh, vl):
        assert t is None or (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous())
    rows = ragged.M if ragged is not None else Bt * T
    assert qh.shape == (rows, 2 * H * 64) and vh.shape[0] == (H * 64 if ragged is not None else Bt * H * 64)
    Tp = vh.shape[1]
    _chk_f32(out)
    oh, ol = (None, None)
    if out_split is not None:
        oh, ol, _ = _pair(out_split, rows if isinstance(out_split, SplitIL) else None, H * 64)
        assert isinstance(out_split, SplitIL) or (out_split[0].is_contiguous() and out_split[0].numel() == rows * H * 64)
    if ragged is not None:
        _lib.check(_lib.load().cvx_attention_f16x3_varlen(qh.data_ptr(), _p(ql), vh.data_ptr(), _p(vl), _p(out), oh, ol, ragged.cu.data_ptr(),
                                                          ragged.n, ragged.max_T, ragged.M, Tp, H, scale, _sp(qk_scale), _sp(v_scale),
                                                          _sp(out_scale), _stream()), "cvx_attention_f16x3_varlen")
    else:
        _lib.check(_lib.load().cvx_attention_f16x3_scaled(qh.data_ptr(), _p(ql), vh.data_ptr(), _p(vl), _p(out), oh, ol,
                                                          Bt, T, Tp, H, scale, _sp(qk_scale), _sp(v_scale), _sp(out_scale), _stream()),
                   "cvx_attention_f16x3")
    return out if out is not None else out_split


ATTENTION_FORMS = ("A", "B", "C", "D", "A1", "B1", "C1")       # (no D1: single-term launches stay on A1, which measured faster)


def attention_form(Bt: int = 0, T: int = 0, H: int = 1, *, single_term: bool = False, ragged=None):
    """Which attention_f16x3 kernel form the library launches for this problem: (name, queries per block, key groups,
    query waves per block), name one of ATTENTION_FORMS (A: one key group; B: three; C: 64-query blocks, four; D: 256-query blocks whose
    four waves own two query sets each, for launches of 512 such blocks and more, same bits per query as A; a trailing 1:
    the single-term twin).  Host arithmetic of the library's own launch rule: no GPU needed.  ragged: a Ragged, or a plain
    list of sequence lengths (Bt, T are then ignored)."""
    if ragged is not None:
        lengths = ragged.lengths if hasattr(ragged, "lengths") else [int(t) for t in ragged]
        n, max_T, rows = len(lengths), max(lengths), sum(lengths)
    else:
        n, max_T, rows = Bt, T, Bt * T
    qb, ks, nw = C.c_int32(), C.c_int32(), C.c_int32()
    form = _lib.load().cvx_attention_f16x3_form(n, max_T, rows, H, int(single_term), C.byref(qb), C.byref(ks), C.byref(nw))
    if form < 0:
        raise ValueError(f"attention_form: no launch has n_seq={n} max_T={max_T} rows={rows} H={H}")
    return ATTENTION_FORMS[form], qb.value, ks.value, nw.value


def geglu(h: torch.Tensor, out: torch.Tensor, F: int) -> torch.Tensor:
    """out[r, c] = h[r, c] * gelu(h[r, F + c]) for c < F, zeros in the padding columns (text2semantic.py:154-157)."""
    _chk_f32(h, out)
    assert h.is_contiguous() and out.is_contiguous() and h.shape[-1] == 2 * F and out.shape[-1] >= F and h.shape[0] == out.shape[0]
    _lib.check(_lib.load().cvx_geglu_f32(h.data_ptr(), out.data_ptr(), h.shape[0], F, out.shape[-1], _stream()), "cvx_geglu_f32")
    return out


def t2s_sample(logits: torch.Tensor, uniforms: torch.Tensor, filter_mode: int = 0, k: int = 1, thres: float = 0.0,
               temperature: float = 1.0, return_kept: bool = False):
    """The filter + Gumbel argmax of one text2semantic decode step on caller-supplied rows (cvx_t2s_sample_f32): logits, uniforms
    [rows, V] fp32 -> int64 tokens [rows] (and the uint8 kept mask [rows, V]).  filter_mode / k / thres: t2s.filter_setting."""
    _chk_f32(logits, uniforms)
    assert logits.ndim == 2 and logits.shape == uniforms.shape and logits.is_contiguous() and uniforms.is_contiguous()
    rows, V = logits.shape
    tokens = torch.empty(rows, dtype=torch.int64, device=logits.device)
    kept = torch.empty(rows, V, dtype=torch.uint8, device=logits.device) if return_kept else None
    _lib.check(_lib.load().cvx_t2s_sample_f32(logits.data_ptr(), uniforms.data_ptr(), rows, V, int(filter_mode), int(k), float(thres),
                                              float(temperature), tokens.data_ptr(), _p(kept), _stream()), "cvx_t2s_sample_f32")
    return (tokens, kept) if return_kept else tokens


def t2s_logprob(logits: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    """log_softmax(logits[r])[tokens[r]] with the decode's log-prob epilogue (cvx_t2s_logprob_f32): logits [rows, V] fp32, tokens int64
    [rows] -> fp32 [rows].  The summation order is fixed: a function of the row alone."""
    _chk_f32(logits)
    assert logits.ndim == 2 and logits.is_contiguous() and tokens.is_cuda and tokens.dtype == torch.int64 and tokens.is_contiguous()
    rows, V = logits.shape
    assert tokens.shape == (rows,)
    out = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _lib.check(_lib.load().cvx_t2s_logprob_f32(logits.data_ptr(), tokens.data_ptr(), rows, V, out.data_ptr(), _stream()), "cvx_t2s_logprob_f32")
    return out


def t2s_prefill_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, cu: torch.Tensor, kbase: torch.Tensor,
                          nk: Optional[torch.Tensor], max_q: int, heads: int, scale: float, causal: bool) -> torch.Tensor:
    """The packed attention of a text2semantic prefill pass (cvx_t2s_prefill_attention_f32; the definition: include/covomix_hip.h):
    query row r of sequence i, at index p = r - cu[i], attends to the key rows kbase[i] + j for j < (p + 1 if causal else nk[i]).
    q [rows, >= heads * 64] and k, v [*, >= heads * 64] are 2-D fp32 views with unit inner stride (column slices of a packed q | k | v
    or k | v buffer; k and v share their row stride); out [rows, heads * 64] contiguous; cu int32 [n + 1], kbase int32 [>= n], nk int32 [n]
    (None when causal) on the device; max_q: the longest sequence (the host's copy of max(cu[i + 1] - cu[i]))."""
    _chk_f32(q, k, v, out)
    I = heads * 64
    rows, n = q.shape[0], cu.numel() - 1
    assert q.ndim == 2 and k.ndim == 2 and v.ndim == 2 and q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1
    assert q.shape[1] == I and k.shape[1] == I and v.shape[1] == I and k.stride(0) == v.stride(0)
    assert out.is_contiguous() and out.shape == (rows, I)
    for t in (cu, kbase, nk):
        assert t is None or (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous())
    assert kbase.numel() >= n and (nk is None or nk.numel() >= n)
    a = _lib.T2SPrefillAttention()
    a.struct_size, a.n, a.heads, a.causal, a.max_q = C.sizeof(_lib.T2SPrefillAttention), n, heads, 1 if causal else 0, int(max_q)
    a.scale, a.rows = float(scale), rows
    a.q, a.ldq, a.k, a.v, a.ldkv, a.out = _p(q), q.stride(0), _p(k), _p(v), k.stride(0), _p(out)
    a.cu, a.kbase, a.nk = _p(cu), _p(kbase), _p(nk)
    _lib.check(_lib.load().cvx_t2s_prefill_attention_f32(C.byref(a), _stream()), "cvx_t2s_prefill_attention_f32")
    return out


def t2s_prefill_guidance(logits: torch.Tensor, null_row: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """In place on the first null_row.numel() rows of logits [R, width]: l[r] = n + (l[r] - n) * scale[r] with n = l[null_row[r]], the
    guided decode step's operation order (cvx_t2s_prefill_guidance_f32); rows with null_row[r] < 0 are left alone."""
    _chk_f32(logits, scale)
    assert logits.ndim == 2 and logits.is_contiguous() and null_row.is_cuda and null_row.dtype == torch.int32 and null_row.is_contiguous()
    rows = null_row.numel()
    assert scale.is_contiguous() and scale.numel() == rows and rows <= logits.shape[0]
    _lib.check(_lib.load().cvx_t2s_prefill_guidance_f32(logits.data_ptr(), null_row.data_ptr(), scale.data_ptr(), rows, logits.shape[1],
                                                        _stream()), "cvx_t2s_prefill_guidance_f32")
    return logits


def t2s_rules(logits: torch.Tensor, history: torch.Tensor, hist_len: torch.Tensor, table: torch.Tensor, eos_id: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The history rules of the text2semantic decode alone (cvx_t2s_rules_f32; the definition: include/covomix_hip.h,
    cvx_t2s_decode_steps_rules), through the decode's device code: logits [rows, V] fp32, history int64 [rows, hist_ld] (row r holds
    hist_len[r] tokens, int32 [rows]), table int32 [rows, 4] (`t2s.rules_rows`) -> the rows the filter would see, fp32 [rows, V]
    (into `out` when given: contiguous [rows, V]).  The inputs are not written."""
    _chk_f32(logits)
    assert logits.ndim == 2 and logits.is_contiguous()
    rows, V = logits.shape
    assert history.is_cuda and history.dtype == torch.int64 and history.ndim == 2 and history.shape[0] == rows and history.is_contiguous()
    assert hist_len.is_cuda and hist_len.dtype == torch.int32 and hist_len.shape == (rows,) and hist_len.is_contiguous()
    assert table.is_cuda and table.dtype == torch.int32 and table.shape == (rows, _lib.T2S_RULES_WORDS) and table.is_contiguous()
    if out is None:
        out = torch.empty(rows, V, dtype=torch.float32, device=logits.device)
    _chk_f32(out)
    assert out.shape == (rows, V) and out.is_contiguous()
    _lib.check(_lib.load().cvx_t2s_rules_f32(logits.data_ptr(), history.data_ptr() if history.shape[1] else None, hist_len.data_ptr(),
                                             table.data_ptr(), rows, V, history.shape[1], int(eos_id), out.data_ptr(), _stream()),
               "cvx_t2s_rules_f32")
    return out


def t2s_beam_select(logits: torch.Tensor, scores: torch.Tensor, finished: torch.Tensor, beam_size: int):
    """One selection step of the beam search (cvx_t2s_beam_select_f32; the algorithm: include/covomix_hip.h): logits [G * B, S, V] fp32, scores
    fp32 [G * B], finished uint8 / bool [G * B] -> (parents int32 [G * B] - the index inside the group -, tokens int64 [G * B, S], token
    log-probs fp32 [G * B, S], scores fp32 [G * B], finished uint8 [G * B]) of the new hypotheses."""
    _chk_f32(logits, scores)
    assert logits.ndim == 3 and logits.is_contiguous() and scores.is_contiguous()
    rows, S, V = logits.shape
    B = int(beam_size)
    assert B >= 1 and rows % B == 0 and scores.shape == (rows,) and finished.shape == (rows,) and finished.is_cuda
    fin = finished.to(torch.uint8).contiguous()
    dev = logits.device
    parents = torch.empty(rows, dtype=torch.int32, device=dev)
    tokens = torch.empty(rows, S, dtype=torch.int64, device=dev)
    lp = torch.empty(rows, S, dtype=torch.float32, device=dev)
    out_sc = torch.empty(rows, dtype=torch.float32, device=dev)
    out_fin = torch.empty(rows, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().cvx_t2s_beam_select_f32(logits.data_ptr(), scores.data_ptr(), fin.data_ptr(), rows // B, B, S, V, parents.data_ptr(),
                                                   tokens.data_ptr(), lp.data_ptr(), out_sc.data_ptr(), out_fin.data_ptr(), _stream()),
               "cvx_t2s_beam_select_f32")
    return parents, tokens, lp, out_sc, out_fin


def t2s_beam_select_rules(logits: torch.Tensor, scores: torch.Tensor, finished: torch.Tensor, beam_size: int, history: torch.Tensor,
                          hist_len: torch.Tensor, table: torch.Tensor):
    """t2s_beam_select under the history rules of beam search (cvx_t2s_beam_select_rules_f32; the definition: include/covomix_hip.h,
    cvx_t2s_beam_rules_steps): history int32 [G * B, S, hist_ld] - what every hypothesis' ancestry took -, hist_len int32 [G * B], table
    int32 [G, 4] (one rules row per group: [2] n-gram size, [3] minimum length).  Same outputs."""
    _chk_f32(logits, scores)
    assert logits.ndim == 3 and logits.is_contiguous() and scores.is_contiguous()
    rows, S, V = logits.shape
    B = int(beam_size)
    assert B >= 1 and rows % B == 0 and scores.shape == (rows,) and finished.shape == (rows,) and finished.is_cuda
    assert history.dtype == torch.int32 and history.ndim == 3 and history.shape[:2] == (rows, S) and history.is_contiguous() and history.is_cuda
    assert hist_len.dtype == torch.int32 and hist_len.shape == (rows,) and hist_len.is_contiguous() and hist_len.is_cuda
    assert table.dtype == torch.int32 and table.shape == (rows // B, _lib.T2S_RULES_WORDS) and table.is_contiguous() and table.is_cuda
    fin = finished.to(torch.uint8).contiguous()
    dev = logits.device
    parents = torch.empty(rows, dtype=torch.int32, device=dev)
    tokens = torch.empty(rows, S, dtype=torch.int64, device=dev)
    lp = torch.empty(rows, S, dtype=torch.float32, device=dev)
    out_sc = torch.empty(rows, dtype=torch.float32, device=dev)
    out_fin = torch.empty(rows, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().cvx_t2s_beam_select_rules_f32(logits.data_ptr(), scores.data_ptr(), fin.data_ptr(), history.data_ptr(),
                                                         hist_len.data_ptr(), table.data_ptr(), rows // B, B, S, V, history.shape[2],
                                                         parents.data_ptr(), tokens.data_ptr(), lp.data_ptr(), out_sc.data_ptr(),
                                                         out_fin.data_ptr(), _stream()), "cvx_t2s_beam_select_rules_f32")
    return parents, tokens, lp, out_sc, out_fin


def dwconv31_gelu_res(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor,
                      Bt: int, T: int, ragged: Optional[Ragged] = None) -> torch.Tensor:
    _chk_f32(x, w, bias, out)
    C_ = x.shape[-1]
    assert x.is_contiguous() and out.is_contiguous() and w.is_contiguous() and w.numel() == C_ * 31
    if ragged is not None:
        assert x.numel() == ragged.M * C_
        _lib.check(_lib.load().cvx_dwconv31_gelu_res_varlen_f32(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                                                ragged.cu.data_ptr(), ragged.n, ragged.max_T, C_, _stream()),
                   "cvx_dwconv31_gelu_res_varlen_f32")
        return out
    _lib.check(_lib.load().cvx_dwconv31_gelu_res_f32(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                                     Bt, T, C_, _stream()), "cvx_dwconv31_gelu_res_f32")
    return out


def gemm_skinny(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, bias=None, act: int = ACT_NONE) -> torch.Tensor:
    """out [M, N] = act(a [M <= 32, K] @ w[N, K].T + bias): the weight-streaming kernel (cvx_gemm_skinny_f32)."""
    _chk_f32(a, w, out, bias)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and tuple(out.shape) == (M, N) and a.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1
    _lib.check(_lib.load().cvx_gemm_skinny_f32(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias), out.data_ptr(), out.stride(0),
                                               M, N, K, act, _stream()), "cvx_gemm_skinny_f32")
    return out


def cfg_combine_axpy(f_c, f_n, y, cond_scale: float, coef: float, out, out2=None, out3=None) -> None:
    _chk_f32(f_c, f_n, y, out, out2, out3)
    n = y.numel()
    assert f_c.numel() == n and out.numel() == n and (f_n is None or f_n.numel() == n)
    for t in (f_c, f_n, y, out, out2, out3):
        assert t is None or t.is_contiguous()
    _lib.check(_lib.load().cvx_cfg_combine_axpy_f32(f_c.data_ptr(), _p(f_n), y.data_ptr(), cond_scale, coef,
                                                    out.data_ptr(), _p(out2), _p(out3), n, _stream()),
               "cvx_cfg_combine_axpy_f32")


def _rk_stage_args(f_c, f_n, y, weights, out, k_prev, k_out, row_scale, out2, out3):
    """the checks both stage kernels share -> (rows, dim, m, host array of the stage pointers, host array of the weights)"""
    _chk_f32(f_c, f_n, y, out, out2, out3, k_out, row_scale, *k_prev)
    n, m = y.numel(), len(k_prev)
    dim = y.shape[-1]
    rows = n // dim if dim else 0
    assert len(weights) == m + 1 and f_c.numel() == n and out.numel() == n and (f_n is None or f_n.numel() == n)
    assert row_scale is None or (row_scale.numel() == rows and row_scale.is_contiguous())
    for t in (f_c, f_n, y, out, out2, out3, k_out, *k_prev):
        assert t is None or (t.is_contiguous() and t.numel() == n)
    kp = (C.c_void_p * max(m, 1))(*[_p(t) for t in k_prev])
    w = (C.c_float * (m + 1))(*[float(x) for x in weights])
    return rows, dim, m, kp, w


def rk_stage(f_c, f_n, y, cond_scale: float, weights, out, *, k_prev=(), k_out=None, row_scale=None, out2=None, out3=None) -> None:
    """CFG combine + one stage of an explicit Runge-Kutta step (cvx_rk_stage_f32): out = y + sum_j k_prev[j] * weights[j] + v * weights[m],
    v = the combined field (also written to k_out when given).  f_c, y, out ... [rows, dim]; weights: m + 1 floats for the m = len(k_prev)
    stored stages and this one (a stage whose weight is 0 may be None); row_scale [rows]: one guidance scale per row."""
    rows, dim, m, kp, w = _rk_stage_args(f_c, f_n, y, weights, out, k_prev, k_out, row_scale, out2, out3)
    _lib.check(_lib.load().cvx_rk_stage_f32(f_c.data_ptr(), _p(f_n), y.data_ptr(), cond_scale, _p(row_scale), kp, w, m, _p(k_out),
                                            out.data_ptr(), _p(out2), _p(out3), rows, dim, _stream()), "cvx_rk_stage_f32")


RK_ERR_ROWS = 32          # CVX_RK_ERR_ROWS of include/covomix_hip.h: rows of one sequence a block of the error-estimate stage owns


class RkErrMap:
    """The block -> (first row, rows, sequence) table of cvx_rk_stage_err_f32 for sequences of the given lengths packed back to back:
    every sequence is cut into chunks of RK_ERR_ROWS rows counted from its own first row (the last one short).  int32 on the host
    (the library checks it against the launch's rows) and on the device (the kernels read it)."""

    def __init__(self, lengths: Sequence[int], device):
        ent = []
        r0 = 0
        for q, L in enumerate(lengths):
            L = int(L)
            if L < 1:
                raise ValueError(f"sequence {q} has {L} rows")
            for c in range(0, L, RK_ERR_ROWS):
                ent.append((r0 + c, min(RK_ERR_ROWS, L - c), q))
            r0 += L
        self.rows, self.n_seq, self.blocks = r0, len(lengths), len(ent)
        self.host = torch.tensor(ent, dtype=torch.int32).reshape(-1, 3).contiguous()
        self.dev = h2d(self.host, device)


def rk_stage_err(f_c, f_n, y, cond_scale: float, weights, err_weights, out, emap: RkErrMap, partials, *, k_prev=(), k_out=None,
                 row_scale=None, out2=None, out3=None) -> None:
    """rk_stage for the last stage of a step, plus the embedded error estimate (cvx_rk_stage_err_f32): per block of `emap` the sums of
    delta^2 and out^2 over its chunk into partials [blocks, 2], delta = sum_j k_prev[j] * err_weights[j] + v * err_weights[m].  A stage
    may be None only when both of its weights are 0."""
    rows, dim, m, kp, w = _rk_stage_args(f_c, f_n, y, weights, out, k_prev, k_out, row_scale, out2, out3)
    _chk_f32(partials)
    assert len(err_weights) == m + 1 and partials.is_contiguous() and partials.numel() == 2 * emap.blocks and emap.dev.device == y.device
    we = (C.c_float * (m + 1))(*[float(x) for x in err_weights])
    _lib.check(_lib.load().cvx_rk_stage_err_f32(f_c.data_ptr(), _p(f_n), y.data_ptr(), cond_scale, _p(row_scale), kp, w, we, m, _p(k_out),
                                                out.data_ptr(), _p(out2), _p(out3), rows, dim, emap.dev.data_ptr(), emap.host.data_ptr(),
                                                emap.blocks, partials.data_ptr(), _stream()), "cvx_rk_stage_err_f32")


def rk_err_finish(partials, emap: RkErrMap, err) -> None:
    """err [steps, sequences, 2] = per (step, sequence) the chunk sums of partials [steps, blocks, 2] in chunk order (cvx_rk_err_finish_f32)"""
    _chk_f32(partials, err)
    steps = err.shape[0]
    assert partials.is_contiguous() and err.is_contiguous() and tuple(err.shape) == (steps, emap.n_seq, 2)
    assert tuple(partials.shape) == (steps, emap.blocks, 2)
    _lib.check(_lib.load().cvx_rk_err_finish_f32(partials.data_ptr(), emap.dev.data_ptr(), emap.blocks, steps, emap.n_seq, err.data_ptr(),
                                                 _stream()), "cvx_rk_err_finish_f32")


def embed_gather(ids: Optional[torch.Tensor], streams: int, table: torch.Tensor, cond: Optional[torch.Tensor],
                 cond_row: Optional[torch.Tensor], cond_dim: int, null_id: int, out: torch.Tensor, M: int) -> torch.Tensor:
    _chk_f32(table, cond, cond_row, out)
    if ids is not None:
        assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == M * streams
    E = table.shape[1]
    assert out.is_contiguous() and out.numel() == M * (streams * E + cond_dim)
    _lib.check(_lib.load().cvx_embed_gather_f32(_p(ids), streams, table.data_ptr(), E, table.shape[0], _p(cond),
                                                _p(cond_row), cond_dim, null_id, out.data_ptr(), M, _stream()),
               "cvx_embed_gather_f32")
    return out


def time_fourier(times: torch.Tensor, w: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    _chk_f32(times, w, out)
    n, half = times.numel(), w.numel()
    assert out.is_contiguous() and out.numel() == n * 2 * half
    _lib.check(_lib.load().cvx_time_fourier_f32(times.data_ptr(), w.data_ptr(), out.data_ptr(), n, half, _stream()),
               "cvx_time_fourier_f32")
    return out


def _items(dst, items) -> None:
    """Fill a cvx_item_lengths field: items = (int32 CUDA tensor of per-item mel frames, mul, add) or None."""
    if items is None:
        dst.item_len_dev, dst.mul, dst.add = None, 0, 0
        return
    t, mul, add = items
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
    dst.item_len_dev, dst.mul, dst.add = t.data_ptr(), int(mul), int(add)


def hifigan_conv1d(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *,
                   cout: int, ksize: int, dil: int = 1, pad: int = 0, up: int = 1, in_slope: float = 1.0,
                   res=None, accum=None, out_scale: float = 1.0, items=None) -> torch.Tensor:
    _chk_f32(x, wp, bias, out, res, accum)
    B, Cin, Lin = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.shape[0] == B and out.shape[1] == cout
    a = ConvArgs()
    a.x, a.B, a.Cin, a.Lin = x.data_ptr(), B, Cin, Lin
    a.Wp, a.bias = wp.data_ptr(), _p(bias)
    a.out, a.Cout, a.Lout = out.data_ptr(), cout, out.shape[2]
    a.ksize, a.dil, a.pad, a.up = ksize, dil, pad, up
    a.in_slope = in_slope
    a.res, a.accum, a.out_scale = _p(res), _p(accum), out_scale
    _items(a.items, items)
    _lib.check(_lib.load().cvx_hifigan_conv1d_f32(C.byref(a), _stream()), "cvx_hifigan_conv1d_f32")
    return out


def hifigan_pack_weight(w: torch.Tensor, transposed: bool) -> torch.Tensor:
    """Host-side packing of a folded conv weight into the kernel's [co_blk][chunk][k][co][16] layout."""
    w = w.detach().to("cpu", torch.float32).contiguous()
    if transposed:
        cin, cout, k = w.shape
    else:
        cout, cin, k = w.shape
    lib = _lib.load()
    n = lib.cvx_hifigan_packed_weight_floats(cout, cin, k)
    wp = torch.empty(n, dtype=torch.float32)
    _lib.check(lib.cvx_hifigan_pack_weight_f32(w.data_ptr(), cout, cin, k, int(transposed), wp.data_ptr()),
               "cvx_hifigan_pack_weight_f32")
    return wp


def hifigan_pack_conv_transpose1d(w: torch.Tensor, stride: int, padding: int) -> torch.Tensor:
    """ConvTranspose1d weight [Cin, Cout, k] -> the phase-major packed weight of cvx_hifigan_conv_transpose1d_f32 (host side)."""
    w = w.detach().to("cpu", torch.float32).contiguous()
    cin, cout, k = w.shape
    lib = _lib.load()
    wp = torch.empty(lib.cvx_hifigan_conv_transpose1d_packed_floats(cout, cin, k, stride, padding), dtype=torch.float32)
    _lib.check(lib.cvx_hifigan_pack_conv_transpose1d_f32(w.data_ptr(), cin, cout, k, stride, padding, wp.data_ptr()),
               "cvx_hifigan_pack_conv_transpose1d_f32")
    return wp


def hifigan_conv_transpose1d(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, cout: int, ksize: int,
                             stride: int, padding: int, in_slope: float = 1.0, amax_bits: Optional[torch.Tensor] = None,
                             items=None) -> torch.Tensor:
    """out = ConvTranspose1d(leaky_relu(x, in_slope)) in polyphase form; amax_bits (int32[1] on the device, zero): receives the
    bit pattern of max|out| (pow2_scale_from_amax turns it into an activation pre-scale and zeroes it)."""
    _chk_f32(x, wp, bias, out)
    B, Cin, Lin = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.shape[0] == B and out.shape[1] == cout
    a = ConvArgs()
    a.x, a.B, a.Cin, a.Lin = x.data_ptr(), B, Cin, Lin
    a.Wp, a.bias = wp.data_ptr(), _p(bias)
    a.out, a.Cout, a.Lout = out.data_ptr(), cout, out.shape[2]
    a.ksize, a.dil, a.pad, a.up = ksize, 1, ksize - 1 - padding, stride
    a.in_slope, a.out_scale = in_slope, 1.0
    _items(a.items, items)
    _lib.check(_lib.load().cvx_hifigan_conv_transpose1d_f32(C.byref(a), _p(amax_bits), _stream()), "cvx_hifigan_conv_transpose1d_f32")
    return out


def pow2_scale_from_amax(amax_bits: torch.Tensor, target: float, scale: torch.Tensor) -> torch.Tensor:
    """scale[0] = 2^round(log2(target / amax)) from the bit pattern a producer kernel left in amax_bits; amax_bits is zeroed."""
    assert amax_bits.is_cuda and amax_bits.dtype == torch.int32 and scale.is_cuda and scale.dtype == torch.float32
    _lib.check(_lib.load().cvx_pow2_scale_from_amax_f32(amax_bits.data_ptr(), float(target), scale.data_ptr(), _stream()),
               "cvx_pow2_scale_from_amax_f32")
    return scale


HIFI_HALO_L = 32        # zero rows in front of position 0 of every channels-last vocoder buffer (>= largest pad, 25)


def hifigan_cl_rows(L: int) -> int:
    """Rows per batch item of a channels-last vocoder buffer for L valid positions."""
    return HIFI_HALO_L + (L + 255) // 256 * 256 + 64


HIFI_NARROW_NP = 64     # stages up to this tile width run one fused kernel per conv pair (intermediate in LDS): no split pairs in HBM


def hifigan_tile(c: int) -> int:
    """Tile width Np of the split-pipe vocoder kernels for c <= 256 channels; a stage's channels-last buffers are that wide."""
    assert 1 <= c <= 256, "the split-pipe vocoder kernels support up to 256 channels"
    return 32 if c <= 32 else 64 if c <= 64 else 128 if c <= 128 else 256


def hifigan_pack_weight_f16x3(w: torch.Tensor):
    """Conv1d weight [Cout, Cin, k] (fp32, on the GPU) -> (w_hi, w_lo, 1/scale, Np, Cp_in): pre-scaled split pair
    packed [Cp_in/32][k][Np][32] for cvx_hifigan_conv1d_f16x3.  Load-time plumbing."""
    cout, cin, k = w.shape
    np_, cp = hifigan_tile(cout), hifigan_tile(cin)          # a stage's buffers are as wide as its output tile, for inputs too
    full = torch.zeros(np_, cp, k, dtype=torch.float32, device=w.device)
    full[:cout, :cin] = w
    packed = full.reshape(np_, cp // 32, 32, k).permute(1, 3, 0, 2).contiguous()      # [chunk][tap][co][ci]
    hi, lo, inv = split_f16(packed)
    return hi, lo, inv, np_, cp


def hifigan_pack_conv_transpose1d_f16x3(w: torch.Tensor, bias: torch.Tensor, stride: int, padding: int, cp_in: Optional[int] = None):
    """ConvTranspose1d weight [Cin, Cout, K] (fp32, on the GPU) -> the stride-1 form of cvx_hifigan_conv_transpose1d_f16x3
    (include/covomix_hip.h): dict(w_hi, w_lo, acc_scale, bias [stride * Np_out], np_out, cp_in, stride, tile_np, taps, pad,
    w_off).  Output position stride*m + r sees kernel taps c + stride*j (c = (r + padding) % stride) at inputs m + a - j
    (a = (r + padding) // stride).  Phases are grouped into column tiles (<= 256 columns, a whole number of phases) so that
    the taps a tile runs but a phase does not see - zero weights, wasted MFMAs - are fewest.  Load-time plumbing."""
    cin, cout, K = w.shape
    s = int(stride)
    assert 1 <= s <= 8
    np_out, cp = hifigan_tile(cout), cp_in or (cin + 31) // 32 * 32  # cp_in: channel count of the input buffers (>= cin, x32)
    assert cp >= cin and cp % 32 == 0
    ph = []                                               # per phase: (c, a, J) - J taps, input offsets a - J + 1 .. a
    for r in range(s):
        q = r + padding
        c, a = q % s, q // s
        ph.append((c, a, max(0, -(-(K - c) // s))))
    def plan(ppt):                                        # tiles of ppt phases: (first phase, lowest offset, taps)
        tiles = []
        for r0 in range(0, s, ppt):
            live = [(a - J + 1, a) for (c, a, J) in ph[r0:r0 + ppt] if J > 0] or [(0, 0)]
            lo, hi = min(l for l, _ in live), max(h for _, h in live)
            tiles.append((r0, lo, hi - lo + 1))
        return tiles
    cands = [ppt for ppt in range(1, s + 1) if s % ppt == 0 and ppt * np_out in (32, 64, 128, 256) and s // ppt <= 8]
    # matrix work of a plan (taps x columns, summed over its tiles) plus a per-tile term for what every extra tile costs
    # whatever its width (its own activation tiles, blocks and epilogues): the narrow layers prefer ONE tile with a zero tap
    ppt = min(cands, key=lambda n: (sum(t[2] * n * np_out + 256 for t in plan(n)), n))
    tiles, tile_np = plan(ppt), ppt * np_out
    blocks, w_off, taps, pads, off = [], [], [], [], 0
    for r0, lo, nt in tiles:
        full = torch.zeros(tile_np, cp, nt, dtype=torch.float32, device=w.device)      # conv1d weight [co, ci, tap]
        for rl in range(ppt):
            c, a, J = ph[r0 + rl]
            for t in range(nt):
                j = a - (lo + t)
                if 0 <= j < J:
                    full[rl * np_out: rl * np_out + cout, :cin, t] = w[:, :, s * j + c].t()
        blocks.append(full.reshape(tile_np, cp // 32, 32, nt).permute(1, 3, 0, 2).contiguous().reshape(-1))   # [chunk][tap][co][ci]
        w_off.append(off); taps.append(nt); pads.append(-lo)
        off += blocks[-1].numel()
    hi, lo_, inv = split_f16(torch.cat(blocks))
    b = torch.zeros(s, np_out, dtype=torch.float32, device=w.device)
    b[:, :cout] = bias.to(w.device).float()
    return dict(w_hi=hi, w_lo=lo_, acc_scale=inv, bias=b.reshape(-1).contiguous(), np_out=np_out, cp_in=cp, stride=s, tile_np=tile_np,
                taps=taps, pad=pads, w_off=w_off, ksize=K, padding=padding)


def hifigan_conv_transpose1d_f16x3(z, pk: dict, B: int, L_in: int, out: torch.Tensor, L_out: int, *, z_scale=None, amax_bits=None,
                                   items=None) -> torch.Tensor:
    """out (fp32 channels-last [B, Lp_out, Np_out]) = ConvTranspose1d of the activation whose split(leaky_relu(.) * z_scale) pair is
    z = (hi, lo) [B, Lp_in, Cp_in]; pk from hifigan_pack_conv_transpose1d_f16x3.  items: valid OUTPUT positions per item."""
    ensure_saturation_bound()
    zh, zl = z
    assert zh.dtype == torch.float16 and zh.is_contiguous() and zl.is_contiguous() and zh.shape == zl.shape
    assert zh.shape[0] == B and zh.shape[2] == pk["cp_in"], (tuple(zh.shape), pk["cp_in"])
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == B and out.shape[2] == pk["np_out"]
    a = _lib.ConvT16Args()
    a.z_hi, a.z_lo = zh.data_ptr(), zl.data_ptr()
    a.B, a.L_in, a.Lp_in, a.Cp_in, a.halo_in = B, L_in, zh.shape[1], pk["cp_in"], HIFI_HALO_L
    a.w_hi, a.w_lo, a.acc_scale, a.bias = pk["w_hi"].data_ptr(), pk["w_lo"].data_ptr(), pk["acc_scale"], pk["bias"].data_ptr()
    a.Np_out, a.stride, a.n_tiles, a.tile_np = pk["np_out"], pk["stride"], len(pk["taps"]), pk["tile_np"]
    for t in range(len(pk["taps"])):
        a.tile_taps[t], a.tile_pad[t], a.tile_w_off[t] = pk["taps"][t], pk["pad"][t], pk["w_off"][t]
    a.out, a.L_out, a.Lp_out, a.halo_out = out.data_ptr(), L_out, out.shape[1], HIFI_HALO_L
    a.z_scale_dev, a.amax_bits_dev = _sp(z_scale), _p(amax_bits)
    _items(a.items, items)
    _lib.check(_lib.load().cvx_hifigan_conv_transpose1d_f16x3(C.byref(a), _stream()), "cvx_hifigan_conv_transpose1d_f16x3")
    return out


def hifigan_split_channels_last(x_cl: torch.Tensor, z, slope: float, z_scale=None) -> None:
    """z = split(leaky_relu(x_cl, slope) * z_scale) over a whole fp32 channels-last buffer."""
    ensure_saturation_bound()
    zh, zl = z
    assert x_cl.dtype == torch.float32 and x_cl.is_contiguous() and zh.dtype == torch.float16 and zh.is_contiguous() and zl.is_contiguous()
    assert zh.shape == x_cl.shape and zl.shape == x_cl.shape and x_cl.numel() % 4 == 0
    _lib.check(_lib.load().cvx_hifigan_split_channels_last(x_cl.data_ptr(), zh.data_ptr(), zl.data_ptr(), x_cl.numel(), slope,
                                                           _sp(z_scale), _stream()), "cvx_hifigan_split_channels_last")


def hifigan_post_channels_last(x_cl: torch.Tensor, C_: int, L: int, w: torch.Tensor, bias: float, out: torch.Tensor, slope: float = 0.01) -> torch.Tensor:
    """hifigan_post reading the channels-last stage output [B, Lp, Np] (C_ valid channels, L valid positions); out [B, 1, L]."""
    _chk_f32(x_cl, w, out)
    B, Lp, np_ = x_cl.shape
    assert x_cl.is_contiguous() and out.is_contiguous() and out.numel() == B * L and w.numel() == C_ * 7
    _lib.check(_lib.load().cvx_hifigan_post_channels_last_f32(x_cl.data_ptr(), w.data_ptr(), float(bias), out.data_ptr(), B, C_, np_, L, Lp,
                                                              HIFI_HALO_L, slope, _stream()), "cvx_hifigan_post_channels_last_f32")
    return out


def amax_pow2_scale(x: torch.Tensor, target: float, scale: torch.Tensor, scratch: torch.Tensor) -> torch.Tensor:
    """scale[0] = 2^round(log2(target / max|x|)) computed on the device (scratch: one int32 element)."""
    _chk_f32(x, scale)
    assert x.is_contiguous() and scale.numel() == 1 and scratch.is_cuda and scratch.dtype == torch.int32 and scratch.numel() >= 1
    _lib.check(_lib.load().cvx_amax_pow2_scale_f32(x.data_ptr(), x.numel(), float(target), scale.data_ptr(), scratch.data_ptr(), _stream()),
               "cvx_amax_pow2_scale_f32")
    return scale


def _fill_conv16(a, z, wpk, bias, B: int, L: int, *, ksize: int, dil: int, res=None, accum=None, out_x=None,
                 out_scale: float = 1.0, out_z=None, z_slope: float = 0.1, z_scale=None, items=None) -> None:
    zh, zl = z
    w_hi, w_lo, inv, np_, cp = wpk
    assert zh.dtype == torch.float16 and zh.is_contiguous() and zl.is_contiguous() and zh.shape == zl.shape
    assert zh.shape[0] == B and zh.shape[2] == cp and bias.numel() == np_
    a.z_hi, a.z_lo = zh.data_ptr(), zl.data_ptr()
    a.B, a.L, a.Lp, a.Cp_in, a.halo_l = B, L, zh.shape[1], cp, HIFI_HALO_L
    a.w_hi, a.w_lo, a.acc_scale, a.bias = w_hi.data_ptr(), w_lo.data_ptr(), inv, bias.data_ptr()
    a.Np, a.ksize, a.dil = np_, ksize, dil
    for t in (res, accum, out_x):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, zh.shape[1], np_))
    a.res, a.accum, a.out_x, a.out_scale = _p(res), _p(accum), _p(out_x), out_scale
    if out_z is not None:
        oh, ol = out_z
        assert oh.dtype == torch.float16 and oh.is_contiguous() and ol.is_contiguous() and tuple(oh.shape) == (B, zh.shape[1], np_)
        a.out_zhi, a.out_zlo = oh.data_ptr(), ol.data_ptr()
    else:
        a.out_zhi, a.out_zlo = None, None
    a.z_slope = z_slope
    a.z_scale_dev = _sp(z_scale)
    _items(a.items, items)


def hifigan_conv1d_f16x3(z, wpk, bias, B: int, L: int, **kw) -> None:
    """z = (hi, lo) channels-last [B, Lp, Cp_in]; wpk from hifigan_pack_weight_f16x3; bias [Np] (zero padded).
    Keywords: ksize, dil, res, accum, out_x, out_scale, out_z, z_slope, z_scale, items."""
    ensure_saturation_bound()
    a = _lib.Conv16Args()
    _fill_conv16(a, z, wpk, bias, B, L, **kw)
    _lib.check(_lib.load().cvx_hifigan_conv1d_f16x3(C.byref(a), _stream()), "cvx_hifigan_conv1d_f16x3")


def hifigan_conv1d_group_f16x3(problems, B: int, L: int) -> None:
    """1..3 independent convolutions of one shape as ONE launch (cvx_hifigan_conv1d_group_f16x3): problems = dicts of the arguments
    of hifigan_conv1d_f16x3 (z, wpk, bias and its keywords); bit-identical to calling it once per problem."""
    ensure_saturation_bound()
    n = len(problems)
    arr = (_lib.Conv16Args * n)()
    for j, pr in enumerate(problems):
        pr = dict(pr)
        _fill_conv16(arr[j], pr.pop("z"), pr.pop("wpk"), pr.pop("bias"), B, L, **pr)
    _lib.check(_lib.load().cvx_hifigan_conv1d_group_f16x3(arr, n, _stream()), "cvx_hifigan_conv1d_group_f16x3")


def hifigan_conv1d_form(np_: int, L: int, B: int, n_problems: int = 1, cus: Optional[int] = None) -> int:
    """Positions per thread block (256, 192 or 160) of the launch hifigan_conv1d_f16x3 / _group_ / the conv-transpose (n_problems = its
    column tiles) make for this shape on a stream of `cus` compute units (default: the current stream's).  The library's own
    launch rule (cvx_hifigan_conv1d_f16x3_form): host arithmetic."""
    rows = _lib.load().cvx_hifigan_conv1d_f16x3_form(np_, L, B, n_problems, stream_cus() if cus is None else int(cus))
    if rows < 0:
        raise ValueError(f"hifigan_conv1d_form: no launch has Np={np_} L={L} B={B} n_problems={n_problems} cus={cus}")
    return rows


def _fill_resblock16(a, x_cl, z, block, B: int, L: int, scratch: dict, accum, out, out_scale: float, z_scale, items) -> None:
    narrow = x_cl.shape[2] <= HIFI_NARROW_NP  # fused pair kernel: z / t / rz0 / rz1 unused
    zh, zl = z if z is not None else (None, None)
    assert narrow or z is not None
    a.x, a.z_hi, a.z_lo = x_cl.data_ptr(), _p(zh), _p(zl)
    a.B, a.L, a.Lp, a.Np, a.halo_l = B, L, x_cl.shape[1], x_cl.shape[2], HIFI_HALO_L
    for m, (c1, c2) in enumerate(block):
        for dst, c in ((a.c1[m], c1), (a.c2[m], c2)):
            w_hi, w_lo, inv, np_, cp = c.w16
            assert np_ == cp == x_cl.shape[2] and c.bias16.numel() == np_
            dst.w_hi, dst.w_lo, dst.acc_scale, dst.bias = w_hi.data_ptr(), w_lo.data_ptr(), inv, c.bias16.data_ptr()
        a.dil[m] = c1.dil
        assert c2.dil == 1 and c1.k == c2.k
    a.ksize = block[0][0].k
    a.xa, a.xb = scratch["r0"].data_ptr(), scratch["r1"].data_ptr()
    if not narrow:
        a.t_hi, a.t_lo = scratch["t"][0].data_ptr(), scratch["t"][1].data_ptr()
        a.za_hi, a.za_lo = scratch["rz0"][0].data_ptr(), scratch["rz0"][1].data_ptr()
        a.zb_hi, a.zb_lo = scratch["rz1"][0].data_ptr(), scratch["rz1"][1].data_ptr()
    a.accum, a.out, a.out_scale = _p(accum), out.data_ptr(), out_scale
    a.z_scale_dev = _sp(z_scale)
    _items(a.items, items)


def hifigan_resblock_f16x3(x_cl, z, block, B: int, L: int, scratch: dict, *, accum=None, out=None, out_scale: float = 1.0, z_scale=None,
                           items=None) -> None:
    """One ResBlock1 (three conv pairs) through the operator-level C entry point cvx_hifigan_resblock_f16x3.
    block: list of 3 (c1, c2) pairs of objects with .w16 = hifigan_pack_weight_f16x3(...), .bias16, .k, .dil;
    scratch: dict with t, rz0, rz1 (split pairs) and r0, r1 (fp32), all [B, Lp, Np] like x_cl / z."""
    ensure_saturation_bound()
    a = _lib.Resblock16Args()
    _fill_resblock16(a, x_cl, z, block, B, L, scratch, accum, out, out_scale, z_scale, items)
    _lib.check(_lib.load().cvx_hifigan_resblock_f16x3(C.byref(a), _stream()), "cvx_hifigan_resblock_f16x3")


def hifigan_resblock_stage_f16x3(x_cl, z, blocks, B: int, L: int, scratches, out, *, out_scale: float = 1.0, z_scale=None, items=None) -> None:
    """out = out_scale * sum_j ResBlock1_j(x) for the (up to 3) ResBlocks of one generator stage (models.py:104-110) through
    cvx_hifigan_resblock_stage_f16x3: the convolutions of different blocks that do not depend on each other share launches; bit-identical
    to calling hifigan_resblock_f16x3 block after block (accum = out from the second block on, out_scale on the last).
    scratches: one scratch dict per block (t, rz0, rz1, r0, r1 - their own buffers)."""
    ensure_saturation_bound()
    n = len(blocks)
    arr = (_lib.Resblock16Args * n)()
    for j, block in enumerate(blocks):
        _fill_resblock16(arr[j], x_cl, z, block, B, L, scratches[j], out if j > 0 else None, out, out_scale if j == n - 1 else 1.0, z_scale, items)
    _lib.check(_lib.load().cvx_hifigan_resblock_stage_f16x3(arr, n, _stream()), "cvx_hifigan_resblock_stage_f16x3")


def hifigan_resblock_pair_f16x3(x_cl, c1, c2, B: int, L: int, out, *, accum=None, out_scale: float = 1.0, z_scale=None, flags: int = 0,
                                items=None) -> None:
    """out = (c2(lrelu(c1(lrelu(x)))) + x (+ accum)) * out_scale as one kernel (cvx_hifigan_resblock_pair_f16x3; Np = 32 / 64).
    x_cl / out / accum: fp32 channels-last [B, Lp, Np]; c1, c2: objects with .w16, .bias16, .k, .dil (c2.dil == 1)."""
    ensure_saturation_bound()
    a = _lib.Respair16Args()
    a.x = x_cl.data_ptr()
    a.B, a.L, a.Lp, a.Np, a.halo_l = B, L, x_cl.shape[1], x_cl.shape[2], HIFI_HALO_L
    for dst, c in ((a.c1, c1), (a.c2, c2)):
        w_hi, w_lo, inv, np_, cp = c.w16
        assert np_ == cp == x_cl.shape[2] and c.bias16.numel() == np_
        dst.w_hi, dst.w_lo, dst.acc_scale, dst.bias = w_hi.data_ptr(), w_lo.data_ptr(), inv, c.bias16.data_ptr()
    assert c2.dil == 1 and c1.k == c2.k
    a.ksize, a.dil = c1.k, c1.dil
    a.accum, a.out, a.out_scale = _p(accum), out.data_ptr(), out_scale
    a.z_scale_dev = _sp(z_scale)
    a.flags = flags
    _items(a.items, items)
    _lib.check(_lib.load().cvx_hifigan_resblock_pair_f16x3(C.byref(a), _stream()), "cvx_hifigan_resblock_pair_f16x3")


def hifigan_to_channels_last(x: torch.Tensor, x_cl: Optional[torch.Tensor], z, slope: float, z_scale=None) -> None:
    """x [B, C, L] fp32 channel-major -> x_cl [B, Lp, Cp] fp32 and / or z = split(leaky_relu(x)) [B, Lp, Cp]."""
    ensure_saturation_bound()
    _chk_f32(x, x_cl)
    B, Cc, L = x.shape
    ref = x_cl if x_cl is not None else z[0]
    Lp, Cp = ref.shape[1], ref.shape[2]
    assert x.is_contiguous() and ref.is_contiguous() and ref.shape[0] == B
    zh, zl = z if z is not None else (None, None)
    _lib.check(_lib.load().cvx_hifigan_to_channels_last_scaled(x.data_ptr(), _p(x_cl), _p(zh), _p(zl), B, Cc, L, Lp, Cp, HIFI_HALO_L,
                                                               slope, _sp(z_scale), _stream()), "cvx_hifigan_to_channels_last")


def hifigan_from_channels_last(x_cl: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    _chk_f32(x_cl, x)
    B, Cc, L = x.shape
    assert x.is_contiguous() and x_cl.is_contiguous() and x_cl.shape[0] == B
    _lib.check(_lib.load().cvx_hifigan_from_channels_last(x_cl.data_ptr(), x.data_ptr(), B, Cc, L, x_cl.shape[1], x_cl.shape[2],
                                                          HIFI_HALO_L, _stream()), "cvx_hifigan_from_channels_last")
    return x


def hifigan_post(x: torch.Tensor, w: torch.Tensor, bias: float, out: torch.Tensor, slope: float = 0.01) -> torch.Tensor:
    _chk_f32(x, w, out)
    B, Cin, L = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.numel() == B * L and w.numel() == Cin * 7
    _lib.check(_lib.load().cvx_hifigan_post_f32(x.data_ptr(), w.data_ptr(), bias, out.data_ptr(), B, Cin, L, slope,
                                                _stream()), "cvx_hifigan_post_f32")
    return out


def wav_to_int16(wav: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk_f32(wav)
    assert wav.is_contiguous()
    if out is None:
        out = torch.empty(wav.shape, dtype=torch.int16, device=wav.device)
    _lib.check(_lib.load().cvx_wav_to_int16(wav.data_ptr(), out.data_ptr(), wav.numel(), _stream()), "cvx_wav_to_int16")
    return out


# ---------------------------------------------------------------- HuBERT tokeniser (N4)
def hubert_conv0_gn_gelu(wav: torch.Tensor, w: torch.Tensor, gn_gamma: torch.Tensor, gn_beta: torch.Tensor,
                         stride: int, eps: float = 1e-5) -> torch.Tensor:
    """First conv layer + GroupNorm(C, C) + GELU of the HuBERT feature extractor: wav [n] -> [L, C] channels-last."""
    _chk_f32(wav, w, gn_gamma, gn_beta)
    assert wav.dim() == 1 and wav.is_contiguous() and w.is_contiguous() and w.dim() == 2
    C, k = w.shape
    n = wav.numel()
    L = (n - k) // stride + 1
    lib = _lib.load()
    out = torch.empty(max(L, 0), C, dtype=torch.float32, device=wav.device)
    ws = torch.empty(int(lib.cvx_hubert_conv0_workspace_floats(max(L, 1), C)), dtype=torch.float32, device=wav.device)
    _lib.check(lib.cvx_hubert_conv0_gn_gelu_f32(wav.data_ptr(), n, w.data_ptr(), C, k, stride, gn_gamma.data_ptr(),
                                                gn_beta.data_ptr(), eps, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "cvx_hubert_conv0_gn_gelu_f32")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: Optional[torch.Tensor] = None,
              eps: float = 1e-5) -> torch.Tensor:
    _chk_f32(x, gamma, beta, out)
    assert x.is_contiguous() and gamma.is_contiguous() and beta.is_contiguous()
    D = x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    assert out.is_contiguous() and out.shape == x.shape
    _lib.check(_lib.load().cvx_layernorm_f32(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                             x.numel() // D, D, eps, _stream()), "cvx_layernorm_f32")
    return out


def hubert_group_pack(x: torch.Tensor, groups: int, halo: int) -> torch.Tensor:
    """x [T, D] -> [groups, T + 2*halo, D/groups] with zero halos (operand of the grouped positional convolution)."""
    _chk_f32(x)
    assert x.dim() == 2 and x.is_contiguous()
    T, D = x.shape
    out = torch.empty(groups, T + 2 * halo, D // groups, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().cvx_hubert_group_pack_f32(x.data_ptr(), out.data_ptr(), T, D, groups, halo, _stream()),
               "cvx_hubert_group_pack_f32")
    return out


def _i32_pair(a, device):
    """A host int32 array and its copy on the device (the ragged HuBERT calls take both: the host words size and validate the
    launch, the kernels read the device words)."""
    host = torch.as_tensor(a, dtype=torch.int32).reshape(-1).contiguous()
    assert host.device.type == "cpu"
    return host, h2d(host, device)


def hubert_conv0_gn_gelu_many(wav: torch.Tensor, w: torch.Tensor, gn_gamma: torch.Tensor, gn_beta: torch.Tensor, stride: int,
                              starts: Sequence[int], rows: Sequence[int], eps: float = 1e-5) -> torch.Tensor:
    """hubert_conv0_gn_gelu over a PACKED waveform with GroupNorm statistics per item: item b owns rows [starts[b], starts[b] +
    rows[b]) of the [L, C] output (in row order, not overlapping); every row of no item comes back zero."""
    _chk_f32(wav, w, gn_gamma, gn_beta)
    assert wav.dim() == 1 and wav.is_contiguous() and w.is_contiguous() and w.dim() == 2 and len(starts) == len(rows) > 0
    C, k = w.shape
    n = wav.numel()
    L = (n - k) // stride + 1
    rows3, chunk = [], 0
    for s0, r in zip(starts, rows):
        rows3 += [int(s0), int(r), chunk]
        chunk += -(-int(r) // 128)
    host, dev = _i32_pair(rows3, wav.device)
    lib = _lib.load()
    out = torch.empty(max(L, 0), C, dtype=torch.float32, device=wav.device)
    need = int(lib.cvx_hubert_conv0_many_workspace_floats(host.data_ptr(), len(starts), C))
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=wav.device)
    _lib.check(lib.cvx_hubert_conv0_gn_gelu_many_f32(wav.data_ptr(), n, w.data_ptr(), C, k, stride, gn_gamma.data_ptr(), gn_beta.data_ptr(),
                                                     eps, host.data_ptr(), dev.data_ptr(), len(starts), out.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), _stream()), "cvx_hubert_conv0_gn_gelu_many_f32")
    return out


def row_gather(x: torch.Tensor, row_map: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = x[row_map[r]] (zeros where row_map[r] < 0); x [R, C] fp32, C % 4 == 0."""
    _chk_f32(x, out)
    assert x.dim() == 2 and x.is_contiguous()
    host, dev = _i32_pair(row_map, x.device)
    assert host.numel() == 0 or int(host.max()) < x.shape[0]
    out = torch.empty(host.numel(), x.shape[1], dtype=torch.float32, device=x.device) if out is None else out
    assert out.is_contiguous() and out.shape == (host.numel(), x.shape[1])
    _lib.check(_lib.load().cvx_row_gather_f32(x.data_ptr(), out.data_ptr(), dev.data_ptr(), host.numel(), x.shape[1], _stream()),
               "cvx_row_gather_f32")
    return out


def hubert_group_pack_many(x: torch.Tensor, groups: int, pack_src: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Ragged hubert_group_pack: x [M, D] -> [groups, len(pack_src), D/groups], row j of every group = x[pack_src[j]]'s slice, zero
    where pack_src[j] < 0 (the items' halos, written on every call)."""
    _chk_f32(x, out)
    assert x.dim() == 2 and x.is_contiguous()
    host, dev = _i32_pair(pack_src, x.device)
    M, D = x.shape
    assert host.numel() > 0 and int(host.max()) < M
    out = torch.empty(groups, host.numel(), D // groups, dtype=torch.float32, device=x.device) if out is None else out
    assert out.is_contiguous() and out.shape == (groups, host.numel(), D // groups)
    _lib.check(_lib.load().cvx_hubert_group_pack_many_f32(x.data_ptr(), out.data_ptr(), dev.data_ptr(), host.numel(), D, groups, _stream()),
               "cvx_hubert_group_pack_many_f32")
    return out


def hubert_group_unpack_add(h: torch.Tensor, conv: torch.Tensor, unpack: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = h[r] + conv[unpack[r]]: the positional convolution's output rows (haloed numbering) back on compact rows."""
    _chk_f32(h, conv, out)
    assert h.dim() == 2 and h.is_contiguous() and conv.is_contiguous() and conv.shape[1] == h.shape[1]
    host, dev = _i32_pair(unpack, h.device)
    assert host.numel() == h.shape[0] and (host.numel() == 0 or (int(host.min()) >= 0 and int(host.max()) < conv.shape[0]))
    out = torch.empty_like(h) if out is None else out
    assert out.is_contiguous() and out.shape == h.shape
    _lib.check(_lib.load().cvx_hubert_group_unpack_add_f32(h.data_ptr(), conv.data_ptr(), dev.data_ptr(), out.data_ptr(), h.shape[0],
                                                           h.shape[1], _stream()), "cvx_hubert_group_unpack_add_f32")
    return out


def kmeans_argmin(x: torch.Tensor, dots: torch.Tensor, cnorm: torch.Tensor, with_margin: bool = False):
    """labels[t] = argmin_j (|x_t|^2 - 2 dots[t, j]) + cnorm[j]  (int64); optionally also the runner-up margin."""
    _chk_f32(x, dots, cnorm)
    assert x.dim() == 2 and x.is_contiguous() and dots.is_contiguous() and cnorm.is_contiguous()
    T, D = x.shape
    K = cnorm.numel()
    assert dots.shape == (T, K)
    labels = torch.empty(T, dtype=torch.int64, device=x.device)
    margin = torch.empty(T, dtype=torch.float32, device=x.device) if with_margin else None
    if T == 0:
        return (labels, margin) if with_margin else labels
    _lib.check(_lib.load().cvx_kmeans_argmin_f32(x.data_ptr(), dots.data_ptr(), cnorm.data_ptr(), labels.data_ptr(),
                                                 _p(margin), T, D, K, _stream()), "cvx_kmeans_argmin_f32")
    return (labels, margin) if with_margin else labels


EDIT_MAX_LEN = _lib.EDIT_MAX_LEN      # tokens per sequence of edit_distance (CVX_EDIT_MAX_LEN)


def edit_distance_tables(lengths: Sequence[int], pairs) -> tuple:
    """The two host tables of cvx_edit_distance_i64 for sequences packed back to back: items int32 [n, 2] (offset, length) and pairs
    int32 [P, 2] (item a, item b).  ValueError for a length outside [0, EDIT_MAX_LEN], a pair that is no (i, j) of two sequence indices,
    or a pool of 2^31 tokens or more."""
    lens = [int(x) for x in lengths]
    for i, n in enumerate(lens):
        if not 0 <= n <= EDIT_MAX_LEN:
            raise ValueError(f"edit_distance: sequence {i} has {n} tokens (0 ... {EDIT_MAX_LEN})")
    if sum(lens) >= 1 << 31:
        raise ValueError(f"edit_distance: {sum(lens)} tokens in one call (fewer than 2^31)")
    offs, off = [], 0
    for n in lens:
        offs.append(off)
        off += n
    items = torch.tensor(list(zip(offs, lens)), dtype=torch.int32).reshape(-1, 2)
    rows = []
    for p, pr in enumerate(pairs):
        if not isinstance(pr, (tuple, list)) or len(pr) != 2 or any(isinstance(x, bool) or not isinstance(x, int) for x in pr):
            raise ValueError(f"edit_distance: pair {p} = {pr!r} is no (i, j) of two sequence indices")
        if not (0 <= pr[0] < len(lens) and 0 <= pr[1] < len(lens)):
            raise ValueError(f"edit_distance: pair {p} = {tuple(pr)} names a sequence outside the {len(lens)} of the call")
        rows.append((pr[0], pr[1]))
    return items, torch.tensor(rows, dtype=torch.int32).reshape(-1, 2)


def edit_distance(sequences, pairs, device=None) -> torch.Tensor:
    """Unit-cost Levenshtein distances (substitution, insertion, deletion: 1 each) between token sequences: out[p] = the distance between
    sequences[i] and sequences[j] of pairs[p] = (i, j); int32 [len(pairs)] on the HOST.  sequences: 1-D int64 tensors of 0 ...
    EDIT_MAX_LEN tokens, on the host or the device; pairs may repeat and may name one sequence twice.  One pooled upload (tokens and
    both tables in one buffer), one launch (cvx_edit_distance_i64: a block per pair), one download.  Tokens are compared by their low 32
    bits; host sequences with a value outside int32 are a ValueError.  No pairs: an empty result and no launch."""
    seqs = list(sequences)
    for i, q in enumerate(seqs):
        if not isinstance(q, torch.Tensor) or q.dtype != torch.int64 or q.dim() != 1:
            raise TypeError(f"edit_distance: sequence {i} must be a 1-D int64 tensor")
    items, prs = edit_distance_tables([q.numel() for q in seqs], pairs)
    if prs.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int32)
    on_dev = [q for q in seqs if q.is_cuda]
    if device is None:
        device = on_dev[0].device if on_dev else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _lib.CovomixHipError("edit_distance needs a GPU: covomix_amd has no CPU path")
    lib = _lib.load()
    n_tok, n_items, n_pairs = int(items[:, 1].sum()), items.shape[0], prs.shape[0]
    tables = torch.cat((items.reshape(-1), prs.reshape(-1)))
    with torch.cuda.device(device):
        if not on_dev:
            # tokens (int64) then the tables (int32 words) in ONE pinned buffer: one copy
            pool = torch.empty(n_tok + (tables.numel() + 1) // 2, dtype=torch.int64).pin_memory()
            if n_tok:
                torch.cat(seqs, out=pool[:n_tok])
                if int(pool[:n_tok].min()) < -(1 << 31) or int(pool[:n_tok].max()) >= 1 << 31:
                    raise ValueError("edit_distance: token values outside int32")
            pool[n_tok:].view(torch.int32)[:tables.numel()] = tables
            pool_dev = pool.to(device, non_blocking=True)
            tok_dev, tab_dev = pool_dev[:n_tok], pool_dev[n_tok:].view(torch.int32)
        else:
            tok_dev = torch.cat([q.to(device) for q in seqs]) if n_tok else torch.zeros(0, dtype=torch.int64, device=device)
            tab_dev = h2d(tables, device)
        out = torch.empty(n_pairs, dtype=torch.int32, device=device)
        _lib.check(lib.cvx_edit_distance_i64(tok_dev.data_ptr(), n_tok, items.data_ptr(), tab_dev.data_ptr(), n_items, prs.data_ptr(),
                                             tab_dev.data_ptr() + 8 * n_items, n_pairs, out.data_ptr(), _stream()), "cvx_edit_distance_i64")
        return out.cpu()


DTW_MAX_FRAMES = _lib.DTW_MAX_FRAMES  # frames per sequence of dtw (CVX_DTW_MAX_FRAMES)
DTW_MAX_DIM = _lib.DTW_MAX_DIM        # features per frame (CVX_DTW_MAX_DIM)


def dtw_tables(lengths: Sequence[int], pairs) -> tuple:
    """The two host tables of cvx_dtw_f32 for feature sequences packed back to back: items int32 [n, 2] (first row, frames) and pairs
    int32 [P, 2] (item a, item b).  ValueError for a length outside [0, DTW_MAX_FRAMES], a pair that is no (i, j) of two sequence
    indices, or a pool of 2^31 rows or more."""
    lens = [int(x) for x in lengths]
    for i, n in enumerate(lens):
        if not 0 <= n <= DTW_MAX_FRAMES:
            raise ValueError(f"dtw: sequence {i} has {n} frames (0 ... {DTW_MAX_FRAMES})")
    if sum(lens) >= 1 << 31:
        raise ValueError(f"dtw: {sum(lens)} frames in one call (fewer than 2^31)")
    rows, row = [], 0
    for n in lens:
        rows.append(row)
        row += n
    items = torch.tensor(list(zip(rows, lens)), dtype=torch.int32).reshape(-1, 2)
    out = []
    for p, pr in enumerate(pairs):
        if not isinstance(pr, (tuple, list)) or len(pr) != 2 or any(isinstance(x, bool) or not isinstance(x, int) for x in pr):
            raise ValueError(f"dtw: pair {p} = {pr!r} is no (i, j) of two sequence indices")
        if not (0 <= pr[0] < len(lens) and 0 <= pr[1] < len(lens)):
            raise ValueError(f"dtw: pair {p} = {tuple(pr)} names a sequence outside the {len(lens)} of the call")
        out.append((pr[0], pr[1]))
    return items, torch.tensor(out, dtype=torch.int32).reshape(-1, 2)


def dtw(features, pairs, device=None) -> tuple:
    """Dynamic time warping between feature sequences: for pairs[p] = (i, j) the cost (sum of the Euclidean frame distances) and the
    length in cells of the best warping path between features[i] and features[j], steps (i-1, j-1), (i-1, j), (i, j-1) at unit weight,
    no window; among the paths of the smallest cost the shortest one is counted.  -> (cost float32 [P], steps int32 [P]) on the HOST.
    The arithmetic is fixed to the bit (include/covomix_hip.h, "DTW").  features: 2-D fp32 tensors [T_i, D] of one D, 1 <= D <=
    DTW_MAX_DIM, 0 <= T_i <= DTW_MAX_FRAMES, on the host or the device; pairs may repeat and may name one sequence twice; a sequence
    without frames gives (0, 0).  One pooled upload (the frames, rows padded to a multiple of 4 floats, and both tables in one buffer),
    one launch (cvx_dtw_f32: a block per pair), one download.  TypeError / ValueError: a wrong dtype or rank, mixed D, a D or a length
    outside the limits, a bad pair, a non-finite value in a HOST feature (device features are not looked at: their pair's result is
    unspecified).  No pairs: empty results and no launch."""
    feats = list(features)
    for i, f in enumerate(feats):
        if not isinstance(f, torch.Tensor) or f.dtype != torch.float32 or f.dim() != 2:
            raise TypeError(f"dtw: sequence {i} must be a 2-D float32 tensor [frames, D]")
    dims = sorted(set(f.shape[1] for f in feats))
    if len(dims) > 1:
        raise ValueError(f"dtw: sequences of different feature sizes {dims} in one call")
    if dims and not 1 <= dims[0] <= DTW_MAX_DIM:
        raise ValueError(f"dtw: {dims[0]} features per frame (1 ... {DTW_MAX_DIM})")
    items, prs = dtw_tables([f.shape[0] for f in feats], pairs)
    for i, f in enumerate(feats):
        if not f.is_cuda and f.numel() and not bool(torch.isfinite(f).all()):
            raise ValueError(f"dtw: sequence {i} holds a non-finite value")
    if prs.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float32), torch.zeros(0, dtype=torch.int32)
    on_dev = [f for f in feats if f.is_cuda]
    if device is None:
        device = on_dev[0].device if on_dev else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _lib.CovomixHipError("dtw needs a GPU: covomix_amd has no CPU path")
    lib = _lib.load()
    D = dims[0]
    ld = (D + 3) // 4 * 4
    n_rows, n_items, n_pairs = int(items[:, 1].sum()), items.shape[0], prs.shape[0]
    tables = torch.cat((items.reshape(-1), prs.reshape(-1)))
    with torch.cuda.device(device):
        if not on_dev:
            # the frames (fp32, rows of ld floats) then the tables (int32 words) in ONE pinned buffer: one copy
            pool = torch.zeros(n_rows * ld + tables.numel(), dtype=torch.float32).pin_memory()
            if n_rows:
                pool[:n_rows * ld].view(n_rows, ld)[:, :D].copy_(torch.cat(feats))
            pool[n_rows * ld:].view(torch.int32).copy_(tables)
            pool_dev = pool.to(device, non_blocking=True)
            frames_dev, tab_dev = pool_dev[:n_rows * ld], pool_dev[n_rows * ld:].view(torch.int32)
        else:
            frames_dev = torch.zeros(max(n_rows, 1), ld, dtype=torch.float32, device=device)
            if n_rows:
                frames_dev[:n_rows, :D] = torch.cat([f.to(device) for f in feats])
            tab_dev = h2d(tables, device)
        out = torch.empty(2 * n_pairs, dtype=torch.int32, device=device)         # cost (fp32 bits) then steps: one download
        _lib.check(lib.cvx_dtw_f32(frames_dev.data_ptr(), n_rows, ld, D, items.data_ptr(), tab_dev.data_ptr(), n_items, prs.data_ptr(),
                                   tab_dev.data_ptr() + 8 * n_items, n_pairs, out.data_ptr(), out.data_ptr() + 4 * n_pairs, _stream()),
                   "cvx_dtw_f32")
        host = out.cpu()
        return host[:n_pairs].view(torch.float32).clone(), host[n_pairs:].clone()


SEQ_NORM_MAX_SEQS = _lib.SEQ_NORM_MAX_SEQS      # sequences of a packed batch with a time per sequence (CVX_SEQ_NORM_MAX_SEQS)
MASKED_MSE_BLOCK = 256                          # rows one thread of cvx_masked_mse_f32's sequence block strides by


def masked_mse_tree_depth(T: int) -> int:
    """Rounded additions above any term of a sequence sum of masked_mse: ceil(T / 256) in a thread, 6 in the wave, 2 across the waves."""
    return (max(int(T), 1) + MASKED_MSE_BLOCK - 1) // MASKED_MSE_BLOCK + 8


def seq_offsets(seqs, rows: int, what: str = "seq_offsets") -> tuple:
    """The host table of the per-sequence kernels: `seqs` is a Ragged or a sequence of n + 1 row offsets -> (int32 tensor [n + 1], n).
    ValueError: fewer than one or more than SEQ_NORM_MAX_SEQS sequences, a negative or decreasing offset, an end behind `rows`."""
    cu = list(seqs.cu_host) if isinstance(seqs, Ragged) else [x for x in seqs]
    if any(isinstance(x, bool) or not isinstance(x, int) for x in cu):
        raise ValueError(f"{what}: row offsets must be python ints")
    n = len(cu) - 1
    if not 1 <= n <= SEQ_NORM_MAX_SEQS:
        raise ValueError(f"{what}: {n} sequences (1 ... {SEQ_NORM_MAX_SEQS})")
    if cu[0] < 0 or any(b < a for a, b in zip(cu, cu[1:])):
        raise ValueError(f"{what}: row offsets must start at 0 or above and never decrease")
    if cu[-1] > rows or rows >= 1 << 31:
        raise ValueError(f"{what}: the sequences end at row {cu[-1]} of {rows} (fewer than 2^31)")
    return torch.tensor(cu, dtype=torch.int32), n


def _seq_host(seqs, rows: int, what: str) -> tuple:
    """(host int32 [n + 1], n) of a Ragged (its own table) or of n + 1 offsets, validated against `rows`"""
    if not isinstance(seqs, Ragged):
        return seq_offsets(seqs, rows, what)
    if not 1 <= seqs.n <= SEQ_NORM_MAX_SEQS:
        raise ValueError(f"{what}: {seqs.n} sequences (1 ... {SEQ_NORM_MAX_SEQS})")
    if seqs.cu_host[-1] > rows or rows >= 1 << 31:
        raise ValueError(f"{what}: the sequences end at row {seqs.cu_host[-1]} of {rows} (fewer than 2^31)")
    return seqs.cu_host_i32, seqs.n


def _seq_dev(seqs, host: torch.Tensor, device, what: str) -> torch.Tensor:
    """the device copy of the table (a Ragged brings its own, which must live with the rows); called last, when every check has passed"""
    if torch.device(device).type != "cuda" or not torch.cuda.is_available():
        raise _lib.CovomixHipError(f"{what} needs a GPU: covomix_amd has no CPU path")
    if not isinstance(seqs, Ragged):
        return h2d(host, device)
    if seqs.cu.device != torch.device(device):
        raise ValueError(f"{what}: the Ragged's offsets are on {seqs.cu.device}, the rows on {device}")
    return seqs.cu


def _rows_f32(t, what: str, width=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
        raise TypeError(f"{what} must be a contiguous 2-D float32 tensor")
    if width is not None and t.shape[1] != width:
        raise ValueError(f"{what} has {t.shape[1]} columns, {width} are needed")
    if t.data_ptr() % 16:
        raise ValueError(f"{what} must be 16-byte aligned")
    return t


def adarmsnorm_seq(x: torch.Tensor, gamma: torch.Tensor, beta: Optional[torch.Tensor], out: Optional[torch.Tensor], seqs,
                   eps: float = 1e-12, out_split=None, split_scale=None):
    """ops.adarmsnorm with ONE gamma / beta row PER SEQUENCE of a packed batch (cvx_adarmsnorm_seq_f32): x [rows, D]; `seqs` a Ragged
    or n + 1 row offsets; gamma, beta [n, D] fp32 with unit column stride and ANY row stride >= D that is a multiple of 4 (both the
    same: views into one [n, depth, 4, D] table).  Rows outside the sequences are not touched.  A sequence's rows are bit-identical to
    adarmsnorm on its slice with its row.  TypeError / ValueError before anything is launched, the outputs untouched."""
    _rows_f32(x, "adarmsnorm_seq: x")
    rows, D = x.shape
    if D % 4:
        raise ValueError(f"adarmsnorm_seq: D = {D} is no multiple of 4")
    host, n = _seq_host(seqs, rows, "adarmsnorm_seq")
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is None and name == "beta":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (n, D) or t.stride(1) != 1:
            raise ValueError(f"adarmsnorm_seq: {name} must be float32 [{n}, {D}] with unit column stride")
        if t.data_ptr() % 16 or (n > 1 and (t.stride(0) < D or t.stride(0) % 4)):
            raise ValueError(f"adarmsnorm_seq: {name} must be 16-byte aligned with a row stride >= D that is a multiple of 4")
    stride = gamma.stride(0) if n > 1 else D
    if beta is not None and n > 1 and beta.stride(0) != stride:
        raise ValueError("adarmsnorm_seq: gamma and beta must have the same row stride")
    if out is None and out_split is None:
        raise ValueError("adarmsnorm_seq: no output")
    if out is not None:
        _rows_f32(out, "adarmsnorm_seq: out", D)
        if out.shape[0] != rows:
            raise ValueError("adarmsnorm_seq: out must have the rows of x")
    dev = _seq_dev(seqs, host, x.device, "adarmsnorm_seq")
    oh, ol = (None, None)
    if out_split is not None:
        ensure_saturation_bound()
        oh, ol, ld = _pair(out_split, rows if isinstance(out_split, SplitIL) else None, D)
        assert isinstance(out_split, SplitIL) or (out_split[0].is_contiguous() and out_split[0].numel() == x.numel())
        assert not isinstance(out_split, SplitIL) or ld == 2 * D, "adarmsnorm_seq: no row stride (a SplitIL view into a wider buffer)"
    _lib.check(_lib.load().cvx_adarmsnorm_seq_f32(x.data_ptr(), gamma.data_ptr(), _p(beta), _p(out), oh, ol, rows, D, host.data_ptr(),
                                                  dev.data_ptr(), n, stride, float(D) ** 0.5, eps, _sp(split_scale), _stream()),
               "cvx_adarmsnorm_seq_f32")
    return out if out is not None else out_split


def cfm_inputs(x1: torch.Tensor, x0: torch.Tensor, cond: torch.Tensor, mask: torch.Tensor, times: torch.Tensor, seqs, sigma: float,
               w: torch.Tensor, flow: Optional[torch.Tensor] = None, cond_in: Optional[torch.Tensor] = None) -> tuple:
    """The inputs of the flow-matching loss evaluation in one launch (cvx_cfm_inputs_f32): with t = times[sequence of the row],
    w = (1 - (1 - sigma) t) x0 + t x1, flow = x1 - (1 - sigma) x0, cond_in = cond with the rows of mask zeroed - individually rounded
    fp32 operations in that order.  x1, x0, w, flow [rows, dim_out]; cond, cond_in [rows, C]; mask bool / uint8 [rows]; times fp32 [n]
    on the device.  -> (w, flow, cond_in).  TypeError / ValueError before anything is launched, the outputs untouched."""
    _rows_f32(x1, "cfm_inputs: x1")
    rows, dim_out = x1.shape
    _rows_f32(x0, "cfm_inputs: x0", dim_out), _rows_f32(cond, "cfm_inputs: cond"), _rows_f32(w, "cfm_inputs: w", dim_out)
    C = cond.shape[1]
    if dim_out % 4 or C % 4 or dim_out < 4 or C < 4:
        raise ValueError(f"cfm_inputs: widths {dim_out} and {C} must be positive multiples of 4")
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 1 or not mask.is_contiguous():
        raise TypeError("cfm_inputs: mask must be a contiguous bool or uint8 tensor [rows]")
    if not isinstance(times, torch.Tensor) or times.dtype != torch.float32 or times.dim() != 1 or not times.is_contiguous():
        raise TypeError("cfm_inputs: times must be a contiguous float32 tensor [sequences]")
    if not (isinstance(sigma, (int, float)) and 0.0 <= float(sigma) <= 1.0):
        raise ValueError(f"cfm_inputs: sigma = {sigma!r} outside [0, 1]")
    host, n = _seq_host(seqs, rows, "cfm_inputs")
    if times.shape[0] != n:
        raise ValueError(f"cfm_inputs: {times.shape[0]} times for {n} sequences")
    if any(t.shape[0] != rows for t in (x0, cond, w, mask)):
        raise ValueError("cfm_inputs: x0, cond, mask and w must have the rows of x1")
    flow = torch.empty_like(x1) if flow is None else _rows_f32(flow, "cfm_inputs: flow", dim_out)
    cond_in = torch.empty_like(cond) if cond_in is None else _rows_f32(cond_in, "cfm_inputs: cond_in", C)
    if flow.shape[0] != rows or cond_in.shape[0] != rows:
        raise ValueError("cfm_inputs: flow and cond_in must have the rows of x1")
    if len({t.device for t in (x1, x0, cond, mask, times, w, flow, cond_in)}) != 1:
        raise ValueError("cfm_inputs: every tensor must be on the same device")
    dev = _seq_dev(seqs, host, x1.device, "cfm_inputs")
    _lib.check(_lib.load().cvx_cfm_inputs_f32(x1.data_ptr(), x0.data_ptr(), cond.data_ptr(), mask.data_ptr(), times.data_ptr(), host.data_ptr(),
                                              dev.data_ptr(), n, rows, dim_out, C, float(sigma), w.data_ptr(), flow.data_ptr(),
                                              cond_in.data_ptr(), _stream()), "cvx_cfm_inputs_f32")
    return w, flow, cond_in


def masked_mse(pred: torch.Tensor, flow: torch.Tensor, mask: torch.Tensor, seqs, err_rows: Optional[torch.Tensor] = None) -> tuple:
    """The masked mean-squared error per sequence (cvx_masked_mse_f32; reference acoustic.py:527-536): err_rows[r] = mean_d (pred - flow)^2,
    loss[s] = (sum of err_rows over the sequence's masked rows) / max(count[s], 1e-5), count[s] = its masked rows; fixed summation
    orders (masked_mse_tree_depth).  pred, flow [rows, dim_out]; mask bool / uint8 [rows].  -> (loss fp32 [n], count int32 [n],
    err_rows fp32 [rows]) on the device; err_rows is written for the rows of the sequences only (a fresh one is zero elsewhere).
    TypeError / ValueError before anything is launched."""
    _rows_f32(pred, "masked_mse: pred")
    rows, dim_out = pred.shape
    _rows_f32(flow, "masked_mse: flow", dim_out)
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 1 or not mask.is_contiguous():
        raise TypeError("masked_mse: mask must be a contiguous bool or uint8 tensor [rows]")
    if flow.shape[0] != rows or mask.shape[0] != rows:
        raise ValueError("masked_mse: flow and mask must have the rows of pred")
    host, n = _seq_host(seqs, rows, "masked_mse")
    if err_rows is None:
        err_rows = torch.zeros(rows, dtype=torch.float32, device=pred.device)
    elif not isinstance(err_rows, torch.Tensor) or err_rows.dtype != torch.float32 or tuple(err_rows.shape) != (rows,) or not err_rows.is_contiguous():
        raise ValueError("masked_mse: err_rows must be a contiguous float32 tensor [rows]")
    if len({t.device for t in (pred, flow, mask, err_rows)}) != 1:
        raise ValueError("masked_mse: every tensor must be on the same device")
    dev = _seq_dev(seqs, host, pred.device, "masked_mse")
    loss = torch.empty(n, dtype=torch.float32, device=pred.device)
    count = torch.empty(n, dtype=torch.int32, device=pred.device)
    _lib.check(_lib.load().cvx_masked_mse_f32(pred.data_ptr(), flow.data_ptr(), mask.data_ptr(), host.data_ptr(), dev.data_ptr(), n, rows, dim_out,
                                              err_rows.data_ptr(), loss.data_ptr(), count.data_ptr(), _stream()), "cvx_masked_mse_f32")
    return loss, count, err_rows
