"""Every instance of the medium-problem GEMM path (csrc/gemm_f16x3_p8m.hip with the epilogues of gemm_p8s_epi.h at two row groups per
wave and PRE = true, and the split-K reductions splitk_reduce_kernel / splitk_reduce_norm_kernel<NW> of gemm_f16x3.hip) at the edges of
its tiles, its K ring, its block-to-tile map and its split-K factors, through ops.gemm and the C ABI.

Style of test_gemm_p8s_epilogue_edges_gpu.py (helpers in gemm_guarded.py): every output and every operand an epilogue or a DMA piece
reads - bias, residual, RoPE tables, scales, the A rows beyond M and columns beyond K1, the W row beyond N - sits at the top left of
a NaN-filled buffer.  The operands are made on the CPU from seeded generators, so the fp64 reference (the product of the
de-quantised pairs hi + lo with an fp64 epilogue) and the fp32 simulation below see the very halves the kernel reads.

Which launch reaches what (gemm_f16x3_impl, launch_gemm_f16x3_p8m, classify_epilogue, splitk_factor_p8m):
  * interleaved A and W with M < 2048 always take the medium kernel; from 2048 rows on CVX_GEMM_FLAG_MEDIUM (8) forces it, and under
    CVX_GEMM_FLAG_NO_MEDIUM (16) it is the fallback when the large kernel declines (a GELU pair that is only 8-byte aligned).
  * N % 64 != 0 (16, 80, 144): classify_epilogue returns EPI_GENERIC whatever the epilogue -> <false, GENERIC> / <true, GENERIC>.
  * N % 64 == 0 (64, 128, 192, 576, 1152):
        bias or nothing, fp32 store                     <false, BIAS>          with A | A2: <true, BIAS>
        residual, fp32 store (+ twin)                   <false, RES>           with A | A2: <true, GENERIC>
        SiLU, or GELU with an fp32 store                <false, GENERIC>
        bias + GELU, pair only, pair 16-byte aligned    <false, GELU_SPLIT, true>   (permuted W tile rows, 16-byte pair stores)
        ... the same pair four halves further on        <false, GELU_SPLIT>         (8-byte aligned only)
        RoPE + V^T (N = 3 H 64), q | k pair aligned     <false, QKV, true>;  four halves further on  <false, QKV>
    (GELU_SPLIT at N % 64 != 0 does not exist: it is classified GENERIC.)
  * split-K (a workspace, no RoPE, ldc % 4 == 0; K-tiles divide, slices of >= 4 tiles for eight and >= 8 tiles for four / two slices,
    tiles x slices <= 128 / 256, K1 on a slice boundary) always runs <false / true, BIAS> on the partial tiles, then
        a norm, N in 256 / 512 / 768 / 1024    splitk_reduce_norm_kernel<1 / 2 / 3 / 4>
        otherwise                              splitk_reduce_kernel
    SPLIT and NORM below list the shapes with their factors (2, 4, 8, the factor-8 one with A | A2); test_gemm_medium_edges.py
    (CPU) holds the restated rule, the library's workspace function and the workspace ops allocates against them -
    otherwise the library runs unsplit without a word.  Every K of the ring tests (K <= 352) and the edge tests (K = 160) stays
    unsplit: fewer than 8 K-tiles per half, and K = 256 (the one count with eight tiles, hence left out) would be cut in two.
  * block-to-tile map: N = 1152 at M = 300 is nine column tiles -> the branch tiles_n * ksplit >= 8 with a grid padded to 16 units,
    seven of them dead; N = 640, K = 512 is five column tiles x two slices = ten units, six dead.

Bounds.  Whole matrix: rel-L2 < 1e-6 (pairs as hi + lo), 2e-6 for the norm pair - the bounds of test_gemm_medium_gpu.py.  What the
arithmetic alone leaves against fp64 (three fp32 products of the same halves on the CPU, the lo x lo term dropped, an fp32 epilogue
with an exact erf, the pair split), worked out for the shapes of this file:
                                                        whole matrix              worst row
    ring, M = 257 N = 192, K = 32 ... 352               0.7e-7 ... 3.3e-7         0.9e-7 ... 4.2e-7   (3.3e-7: K = 352 with no bias)
    edges, M = 1 ... 129, N = 16 ... 192, K = 160       0.4e-7 ... 2.3e-7         0.4e-7 ... 6.4e-7   (fp32 stores and twins, SiLU / GELU)
    ... their GELU pairs                                0.5e-7 ... 2.1e-7         0.5e-7 ... 3.6e-7
    QKV, M = 1 ... 129, H = 1, 2, K = 160               1.1e-7 ... 2.3e-7         1.1e-7 ... 3.3e-7
    map, N = 1152 K = 96 and N = 640 K = 512            1.1e-7 ... 2.0e-7         1.3e-7 ... 2.4e-7
    split-K, K = 576 ... 1152 (GELU pairs included)     1.7e-7 ... 3.0e-7         2.2e-7 ... 5.1e-7
    norm, N = 256 ... 1024: h and its twin              1.7e-7 ... 2.1e-7         1.8e-7 ... 2.4e-7
    ... the norm pair                                   1.3e-7 ... 2.2e-7         1.6e-7 ... 2.9e-7
    2049 ... 2177 rows, N = 576, K = 96                 1.0e-7 ... 1.7e-7         1.4e-7 ... 2.2e-7
so the floor stays within a third of the bound everywhere, and the rest is for the kernel's summation order and its erf
polynomial.  Worst single row (a whole-matrix norm dilutes an error confined to one row or one 16-column tile): three
times the worst row of the same simulation ON THE SAME OPERANDS, computed on the CPU inside the test - never from what the GPU
returns.  Each launch prints its four figures."""
import math

import pytest
import torch

import gemm_guarded as gg
from gemm_guarded import Guarded, Pair, PairIL, Problem, act_fn, dev, errors, pair_value, splitk_factor_p8m, vec

pytestmark = pytest.mark.gpu

MEDIUM, NO_MEDIUM = 8, 16
TOL, TOL_NORM = 1e-6, 2e-6
GELU, SILU = 1, 2

# (M, N, K, K1, slices): what splitk_factor_p8m gives; `slices` is asserted, not assumed
SPLIT = [(300, 80, 1024, 0, 8), (300, 256, 1024, 384, 8), (300, 512, 1152, 0, 4), (300, 256, 576, 0, 2)]
NORM = [(300, 256, 1024, 0, 8), (300, 512, 1152, 0, 4), (300, 768, 576, 0, 2), (300, 1024, 512, 0, 2)]
MAP = [(300, 1152, 96, 0, 1), (300, 640, 512, 0, 2)]
RING_NK = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11]
RING_A2 = [(nk, k1t) for nk in (6, 11) for k1t in (1, 2, 3, 5)]
EDGE_M = [1, 17, 31, 127, 128, 129]
EDGE_K = 160
UNSPLIT = ([(257, 192, 32 * nk, 0, 1) for nk in RING_NK] + [(257, 192, 32 * nk, 32 * k1t, 1) for nk, k1t in RING_A2] +
           [(M, N, EDGE_K, K1, 1) for M in EDGE_M for N in (16, 64, 80, 128, 144, 192) for K1 in (0, 96)] + [(300, 128, 96, 0, 1)])


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import covomix_amd.ops as o
    assert o._splitk_workspace(dev()).numel() == gg.WORKSPACE_FLOATS
    return o


def _hold(tag, got, ref, sim, tol=TOL):
    """the whole-matrix bound, and the worst row against three times the worst row the arithmetic alone leaves"""
    e, er = errors(got, ref)
    se, ser = errors(sim, ref)
    print(f"FIGURE {tag}: rel-L2 {e:.3e} (arithmetic alone {se:.3e}), worst row {er:.3e} (arithmetic alone {ser:.3e})")
    assert e < tol, (tag, e)
    assert er < 3 * ser, (tag, "worst row", er, ser)


class _P(Problem):
    """+ a bias and a residual, on the CPU and guarded on the GPU"""

    def __init__(self, ops, M, N, K, K1=0, seed=0):
        super().__init__(ops, M, N, K, K1, seed)
        self.b, self.r = self.randn(N), self.randn(M, N)
        self.bias, self.res = vec(N, self.b.to(dev())), Guarded(M, N, data=self.r.to(dev()))


def _one(v):
    """a one-element device scale with NaN behind it"""
    return None if v is None else vec(1, torch.tensor([float(v)], device=dev()))


def _run(ops, P, tag, *, bias=True, act=0, res=False, twin=None, shift=0, write_f32=True, c_scale=None):
    """one launch: outputs guarded, held against fp64 and the simulation -> {name: clone} of the live regions"""
    M, N = P.M, P.N
    c = Guarded(M, N)
    t = PairIL(ops, M, N) if twin == "il" else Pair(M, N, shift=shift) if twin == "pair" else None
    ops.gemm(P.x, P.w, c.v, bias=P.bias if bias else None, act=act, residual=P.res.v if res else None,
             out_split=t.pair if t else None, write_f32=write_f32, c_scale=_one(c_scale), **P.kw)
    ref = act_fn(P.ref + (P.b.double() if bias else 0.0), act) + (P.r.double() if res else 0.0)
    sim = act_fn(P.sim + P.b if bias else P.sim, act)
    sim = sim + P.r if res else sim
    assert sim.dtype == torch.float32
    tag = f"{tag} M={M} N={N} K={P.K} K1={P.K1}"
    out = {}
    if write_f32:
        _hold(tag + " c", c.v, ref, sim)
        assert c.guards_untouched(), tag
        out["c"] = c.v.clone()
    else:
        assert c.unwritten(), tag
    if t is not None:
        cs = float(c_scale or 1.0)
        _hold(tag + " pair", t.value() / cs, ref, pair_value(sim, cs))
        assert t.guards_untouched(), tag
        out["hi"], out["lo"] = (h.clone() for h in t.halves())
    assert P.res.guards_untouched() and P.operands_untouched(), tag
    return out


def _same_bits(a, b, tag):
    assert a.keys() == b.keys() and len(a) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), (tag, k)


# ---------------------------------------------------------------------------------------------------- 1. ring and parity

@pytest.mark.parametrize("nk", RING_NK)
def test_ring_and_parity(ops, nk):
    """Three row tiles (the last with one live row), two column tiles (the second half empty); the K-tile counts at which the ring of
    five buffers first wraps, the parity groups get unequal shares and the t + 4 prefetch turns into dummy pieces.  Twice: equal bits."""
    P = _P(ops, 257, 192, 32 * nk, seed=100 + nk)
    for tag, kw in (("bias", {}), ("plain", dict(bias=False)), ("res", dict(res=True))):
        first = _run(ops, P, f"ring {tag}", **kw)
        _same_bits(first, _run(ops, P, f"ring {tag} again", **kw), (tag, nk))


@pytest.mark.parametrize("nk,k1t", RING_A2)
def test_ring_switches_to_a2_at_odd_and_even_tiles(ops, nk, k1t):
    """A | A2 (<true, BIAS>) switching at K-tile 1, 2, 3, 5: in group 1's and in group 0's tile sequence.  lda_h > 2 K1 with NaN in the
    padding: a switch that is off by one tile reads NaN.  The K order does not depend on where A ends, so the bits equal those of the
    same operands as one A."""
    P2 = _P(ops, 257, 192, 32 * nk, K1=32 * k1t, seed=200 + nk)
    first = _run(ops, P2, "ring a2")
    _same_bits(first, _run(ops, P2, "ring a2 again"), (nk, k1t))
    _same_bits(first, _run(ops, _P(ops, 257, 192, 32 * nk, seed=200 + nk), "ring a2 as one A"), (nk, k1t, "one A"))


# ---------------------------------------------------------------------------------------------------- 2. every instance at the edges

@pytest.mark.parametrize("M", EDGE_M)
def test_row_epilogues_at_row_and_column_edges(ops, M):
    """M < 32: every DMA row clamps to M - 1 and group 1's rows 32-63 of every wave tile are dead; 127 / 128 / 129 around one row tile.
    N = 16 ... 192: partial wave tiles, a half-empty column tile (the instance each N reaches: module docstring)."""
    for N in (16, 80, 128, 144, 192):
        P = _P(ops, M, N, EDGE_K, seed=M * 7 + N)
        tw = "il" if N % 32 == 0 else "pair"
        _run(ops, P, "edge bias")
        _run(ops, P, "edge res", res=True)
        _run(ops, P, "edge silu", act=SILU)
        _run(ops, P, "edge gelu f32", act=GELU)
        _run(ops, P, "edge res twin", res=True, twin=tw)
        _run(ops, P, "edge gelu res twin", act=GELU, res=True, twin=tw)
    for N in (64, 192):
        P = _P(ops, M, N, EDGE_K, seed=M * 7 + N)
        perm = _run(ops, P, "edge gelu_split permuted", act=GELU, twin="pair", write_f32=False)
        plain = _run(ops, P, "edge gelu_split 8-byte", act=GELU, twin="pair", shift=4, write_f32=False)
        _same_bits(perm, plain, (M, N, "gelu_split permuted / not"))       # same K order, group split and exchange sum per element
        _run(ops, P, "edge gelu_split interleaved", act=GELU, twin="il", write_f32=False)
    for N in (80, 192):           # <true, GENERIC>: A | A2 with bias, residual and a split twin; <true, BIAS> beside it
        P = _P(ops, M, N, EDGE_K, K1=96, seed=M * 7 + N)
        _run(ops, P, "edge a2 res twin", res=True, twin="il" if N % 32 == 0 else "pair")
        _run(ops, P, "edge a2 bias")


def _qkv(ops, P, Bt, T, H, shift):
    M, rc, rows = Bt * T, 2 * H * 64, Bt * H * 64
    ang = torch.arange(T).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64)))[None, :]
    cos, sin = ang.cos(), ang.sin()

    def table(t):                # exactly [T, 32] inside a NaN buffer
        flat = torch.full((T * 32 + 64,), gg.NAN, device=dev())
        flat[:T * 32] = t.flatten().to(dev())
        return flat[:T * 32].view(T, 32)
    qk = Pair(M, rc, shift=shift)
    Tp = (T + 31) // 32 * 32
    vt = [torch.zeros(rows + 64, Tp, dtype=torch.float16, device=dev()) for _ in range(2)]
    for v in vt:
        v[rows:] = gg.NAN
    c = Guarded(M, P.N)
    ops.gemm(P.x, P.w, c.v, rope=(table(cos), table(sin)), rope_cols=rc, out_split=qk.pair, vt_split=(vt[0][:rows], vt[1][:rows]),
             write_f32=False, **P.kw)
    tag = f"qkv Bt={Bt} T={T} H={H} shift={shift}"

    def rotate(z):
        zq = z[:, :rc].reshape(Bt, T, 2 * H, 64)
        c_, s_ = torch.cat((cos, cos), -1).to(z.dtype), torch.cat((sin, sin), -1).to(z.dtype)
        rot = torch.cat((-zq[..., 32:], zq[..., :32]), -1)
        return (zq * c_[None, :, None, :] + rot * s_[None, :, None, :]).reshape(M, rc)
    _hold(tag + " q|k", qk.value(), rotate(P.ref), pair_value(rotate(P.sim)))
    assert qk.guards_untouched() and c.unwritten() and P.operands_untouched(), tag
    slots = torch.tensor([gg.vt_slot(t) for t in range(T)])
    assert torch.equal(slots, ops.vt_frame_slots(T, dev()).cpu())
    got = (vt[0][:rows].double() + vt[1][:rows].double()).cpu()[:, slots]                        # [(b, h, d), t] -> [(b, t), (h, d)]
    got = got.reshape(Bt, H, 64, T).permute(0, 3, 1, 2).reshape(M, H * 64)
    _hold(tag + " v^t", got, P.ref[:, rc:], pair_value(P.sim[:, rc:]))
    free = torch.ones(Tp, dtype=torch.bool)
    free[slots] = False
    for v in vt:
        assert bool(torch.isnan(v[rows:]).all()), tag
        assert not bool(free.any()) or float(v[:rows].cpu()[:, free].float().abs().max()) == 0.0, tag
    return dict(qh=qk.h.v.clone(), ql=qk.l.v.clone(), vh=vt[0][:rows].clone(), vl=vt[1][:rows].clone())


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("Bt,T", [(1, 1), (1, 17), (1, 31), (1, 127), (2, 64), (3, 43)])
def test_qkv_permuted_and_not(ops, Bt, T, H):
    """to_qkv at M = Bt T in 1 ... 129: a row tile that straddles sequences, T % 4 != 0, whole 16-frame groups (T = 64); H = 1 leaves the
    V column tile half empty.  The q | k pair 16-byte aligned (<false, QKV, true>) and four halves further on (<false, QKV>): same bits."""
    P = Problem(ops, Bt * T, 3 * H * 64, EDGE_K, seed=Bt * 1000 + T + H)
    _same_bits(_qkv(ops, P, Bt, T, H, 0), _qkv(ops, P, Bt, T, H, 4), (Bt, T, H))


# ---------------------------------------------------------------------------------------------------- 3. map branches

@pytest.mark.parametrize("M,N,K,K1,slices", MAP)
def test_block_to_tile_map_with_dead_units(ops, M, N, K, K1, slices):
    assert splitk_factor_p8m(M, N, K, K1) == slices and len(range(0, N, 128)) * slices in (9, 10)
    P = _P(ops, M, N, K, seed=N)
    _run(ops, P, "map res", res=True)
    _run(ops, P, "map bias")


# ---------------------------------------------------------------------------------------------------- 4. split-K and the plain reduction

@pytest.mark.parametrize("M,N,K,K1,slices", SPLIT)
def test_splitk_reduction_epilogues(ops, M, N, K, K1, slices):
    """splitk_reduce_kernel behind 2, 4 and 8 slices (one of them A | A2 with K1 on a slice boundary): bias only, SiLU, GELU + residual +
    twin, GELU + split only as a plain pair with ldc_h > N, and a c_scale on the pair; ldc > N and ldr > N throughout."""
    assert splitk_factor_p8m(M, N, K, K1) == slices > 1
    P = _P(ops, M, N, K, K1=K1, seed=N + K)
    tw = "il" if N % 32 == 0 else "pair"
    _run(ops, P, f"splitk x{slices} bias")
    _run(ops, P, f"splitk x{slices} silu", act=SILU)
    _run(ops, P, f"splitk x{slices} gelu res twin", act=GELU, res=True, twin=tw)
    _run(ops, P, f"splitk x{slices} gelu split only", act=GELU, twin="pair", write_f32=False)
    first = _run(ops, P, f"splitk x{slices} res twin c_scale", res=True, twin=tw, c_scale=4.0)
    _same_bits(first, _run(ops, P, f"splitk x{slices} res twin c_scale again", res=True, twin=tw, c_scale=4.0), (N, K))


# ---------------------------------------------------------------------------------------------------- 5. norm reduction

def _norm_ref(h, gam, beta, N, eps=1e-12):
    inv = math.sqrt(N) / h.norm(dim=-1, keepdim=True).clamp_min(eps)
    y = h * inv * gam
    return y + beta if beta is not None else y


def _norm_sim(h, gam, beta, N, eps=1e-12):
    inv = torch.tensor(float(N)).sqrt() / (h * h).sum(-1, keepdim=True).sqrt().clamp_min(eps)
    y = h * inv * gam
    return y + beta if beta is not None else y


@pytest.mark.parametrize("M,N,K,K1,slices", NORM)
def test_norm_reduction(ops, M, N, K, K1, slices):
    """splitk_reduce_norm_kernel<1 ... 4>: beta or none, Y interleaved or plain, a device scale or none, a twin or none.  The same bits as
    ops.gemm followed by ops.adarmsnorm, and against fp64.  Row Z of h is exactly zero (the residual is minus what a first run
    stored there): the eps clamp."""
    assert splitk_factor_p8m(M, N, K, K1) == slices > 1 and N % 256 == 0 and N <= 1024       # norm_done: the norm rides in the reduction
    P = _P(ops, M, N, K, seed=N)
    Z = 131
    gam, bet = P.randn(N), P.randn(N)
    gamma, beta_d = vec(N, gam.to(dev())), vec(N, bet.to(dev()))
    c = Guarded(M, N, pad=0)
    P.res.v[Z] = 0.0
    ops.gemm(P.x, P.w, c.v, bias=P.bias, residual=P.res.v, **P.kw)
    P.res.v[Z] = -c.v[Z]
    P.r[Z] = P.res.v[Z].cpu()
    h_ref, h_sim = P.ref + P.b.double() + P.r.double(), P.sim + P.b + P.r
    h_ref[Z], h_sim[Z] = 0.0, 0.0                      # exact in the kernel by construction (asserted below), not in another summation order
    for has_beta, y_il, scale, twin in ((True, True, 4.0, True), (False, False, None, False), (False, True, None, True), (True, False, 4.0, False)):
        tag = f"norm N={N} x{slices} beta={has_beta} il={y_il} scale={scale} twin={twin}"
        mk = (lambda: PairIL(ops, M, N, pad=0)) if y_il else (lambda: Pair(M, N, pad=0))
        c0, c1, y0, y1 = Guarded(M, N, pad=0), Guarded(M, N, pad=0), mk(), mk()
        t0, t1 = (PairIL(ops, M, N), PairIL(ops, M, N)) if twin else (None, None)
        sc = _one(scale)
        beta = beta_d if has_beta else None
        kw = dict(bias=P.bias, residual=P.res.v, **P.kw)
        ops.gemm(P.x, P.w, c0.v, out_split=t0.pair if twin else None, **kw)
        ops.adarmsnorm(c0.v, gamma, beta, None, out_split=y0.pair, split_scale=sc)
        ops.gemm(P.x, P.w, c1.v, out_split=t1.pair if twin else None, norm=dict(gamma=gamma, beta=beta, out_split=y1.pair, scale=sc), **kw)
        assert torch.equal(c0.v, c1.v) and (not twin or torch.equal(t0.v, t1.v)), tag
        assert all(torch.equal(p, q) for p, q in zip(y0.halves(), y1.halves())), tag
        assert c1.guards_untouched() and y1.guards_untouched() and (not twin or t1.guards_untouched()), tag
        assert P.res.guards_untouched() and P.operands_untouched(), tag
        ys = scale or 1.0
        b64, b32 = (bet.double(), bet) if has_beta else (None, None)
        _hold(tag + " c", c1.v, h_ref, h_sim)
        if twin:
            _hold(tag + " twin", t1.value(), h_ref, pair_value(h_sim))
        _hold(tag + " y", y1.value() / ys, _norm_ref(h_ref, gam.double(), b64, N), pair_value(_norm_sim(h_sim, gam, b32, N), ys), TOL_NORM)
        assert float(c1.v[Z].abs().max()) == 0.0, tag
        want_z = pair_value(bet, ys) if has_beta else torch.zeros(N, dtype=torch.float64)
        assert torch.equal((y1.value() / ys)[Z].cpu(), want_z), tag


# ---------------------------------------------------------------------------------------------------- 6. 2048 rows and more

@pytest.mark.parametrize("M", [2049, 2177])
def test_forced_medium_kernel_from_2048_rows(ops, M):
    """CVX_GEMM_FLAG_MEDIUM: 17 / 18 row tiles (one live row / one full tile behind 2048), N = 576 (the fifth column tile half empty)."""
    P = _P(ops, M, 576, 96, seed=M)
    with ops.gemm_flags(MEDIUM):
        _run(ops, P, "forced res twin", res=True, twin="il")
        _run(ops, P, "forced gelu_split", act=GELU, twin="pair", write_f32=False)


def test_fallback_from_the_large_kernel(ops):
    """Under CVX_GEMM_FLAG_NO_MEDIUM the large kernel is asked first; it declines a GELU pair that is only 8-byte aligned, and the
    medium kernel's <false, GELU_SPLIT> takes the launch: the bits of the forced medium kernel's permuted instance on the aligned pair."""
    P = _P(ops, 2100, 576, 96, seed=2100)
    with ops.gemm_flags(NO_MEDIUM):
        fell = _run(ops, P, "fallback gelu_split 8-byte", act=GELU, twin="pair", shift=4, write_f32=False)
    with ops.gemm_flags(MEDIUM):
        _same_bits(fell, _run(ops, P, "forced gelu_split permuted", act=GELU, twin="pair", write_f32=False), "fallback")


# ---------------------------------------------------------------------------------------------------- 7. saturation flag

def _flagged(ops, fn):
    ops.saturation_reset()
    fn()
    return ops.saturation_query()


def _clamped(pair):
    return all(bool(torch.isfinite(h.float()).all()) for h in pair.halves()) and float(pair.halves()[0].float().abs().max()) == 65504.0


@pytest.mark.parametrize("M,N,K,slices", [(300, 128, 96, 1), (300, 256, 576, 2)])
def test_flag_from_the_medium_kernels_and_the_reductions_split_store(ops, M, N, K, slices):
    """(a) the medium kernel's own split store (no split-K), (b) splitk_reduce_kernel's: flag down inside the window, up with
    c_scale = 2^17, the halves clamped to 65504 and not inf."""
    assert splitk_factor_p8m(M, N, K) == slices
    P = _P(ops, M, N, K, seed=7)
    c, t = Guarded(M, N), PairIL(ops, M, N)
    kw = dict(bias=P.bias, residual=P.res.v, out_split=t.pair, **P.kw)
    assert _flagged(ops, lambda: ops.gemm(P.x, P.w, c.v, **kw)) == 0
    assert not _clamped(t)
    assert _flagged(ops, lambda: ops.gemm(P.x, P.w, c.v, c_scale=_one(2.0 ** 17), **kw)) != 0
    assert _clamped(t) and t.guards_untouched() and c.guards_untouched()
    assert _flagged(ops, lambda: ops.gemm(P.x, P.w, c.v, **kw)) == 0


def test_flag_from_the_norm_reductions_two_split_stores(ops):
    """(c) splitk_reduce_norm_kernel: the Y pair (norm scale) and the twin (c_scale), each on its own."""
    M, N, K = 300, 256, 1024
    assert splitk_factor_p8m(M, N, K) == 8
    P = _P(ops, M, N, K, seed=8)
    gamma = vec(N, (1.0 + 0.3 * P.randn(N)).to(dev()))
    c, t, y = Guarded(M, N, pad=0), PairIL(ops, M, N), PairIL(ops, M, N, pad=0)

    def run(y_scale, c_scale):
        return _flagged(ops, lambda: ops.gemm(P.x, P.w, c.v, bias=P.bias, residual=P.res.v, out_split=t.pair, c_scale=_one(c_scale),
                                              norm=dict(gamma=gamma, beta=None, out_split=y.pair, scale=_one(y_scale)), **P.kw))
    assert run(4.0, 4.0) == 0 and not _clamped(y) and not _clamped(t)
    assert run(2.0 ** 17, 4.0) != 0 and _clamped(y) and not _clamped(t)
    assert run(4.0, 2.0 ** 17) != 0 and _clamped(t) and not _clamped(y)
    assert run(None, None) == 0
    assert y.guards_untouched() and t.guards_untouched() and c.guards_untouched()


# ---------------------------------------------------------------------------------------------------- 8. refusals

def test_refusals_launch_nothing(ops):
    """Host-side: N % 16 != 0, and RoPE with N % 64 != 0, on interleaved operands -> CovomixHipError, the pre-filled output untouched."""
    from covomix_amd._lib import CovomixHipError
    P = Problem(ops, 300, 72, 96, seed=1)
    c = Guarded(300, 72)
    with pytest.raises(CovomixHipError):
        ops.gemm(P.x, P.w, c.v, **P.kw)
    P = Problem(ops, 300, 176, 96, seed=2)
    c2, qk = Guarded(300, 176), Pair(300, 176)
    cos, sin = torch.ones(300, 32, device=dev()), torch.zeros(300, 32, device=dev())
    with pytest.raises(CovomixHipError):
        ops.gemm(P.x, P.w, c2.v, rope=(cos, sin), rope_cols=128, **P.kw)
    with pytest.raises(CovomixHipError):
        ops.gemm(P.x, P.w, c2.v, rope=(cos, sin), rope_cols=128, out_split=qk.pair, write_f32=False, **P.kw)
    torch.cuda.synchronize()
    assert c.unwritten() and c2.unwritten() and qk.h.unwritten() and qk.l.unwritten()
