"""GPU: every row epilogue of the large-problem GEMM kernel (gemm_f16x3_p8s.hip, epilogue_rows in gemm_p8s_epi.h) at the edges of its
tiles, in BOTH tile heights.  The edge tests at 2,100-2,304 rows in test_kernels_gpu.py mostly reach the 192-row instances (the launcher's
cost rule picks them there); here every case runs pinned to 256-row tiles (flags 16 | 128) and to 192-row tiles (16 | 64), the two must
agree bit for bit, and each is held against fp64 on the de-quantised operand pairs with the bound of the existing large-kernel tests
(rel-L2 < 1e-6).

Epilogues: res (bias + fp32 residual + fp32 store + twin), res_tw (fp32 residual, gamma on the twin, row sums of squares; and the pair
residual read and written IN PLACE, no fp32 store), bias_tw (A | A2 with two pre-scales), gelu_split, gelu_rs (a factor per row), bias.
Shapes: M = 2048 (a full last panel), 2049 (one live row in the last panel), 2303 (one dead row); N = 512 and 576 (the third
256-column tile has one wave tile inside N and three past it); K = 64 (two K-tiles: the persistent path) and 96 (three: one tile per
block).  Every output and every operand an epilogue reads is a view into a wider, taller buffer (row stride > width, one guard row,
guard columns / elements) pre-filled with NaN: a stray store shows as a finite guard element, a stray load that reaches a result as a NaN.

What the arithmetic itself leaves against fp64 at these shapes (worked out on a CPU: the three fp32 products of the same pairs - the
lo x lo term is dropped, as in the kernel - an fp32 epilogue with an exact erf, the pair split): fp32 stores 0.9e-7 ... 1.3e-7, pairs
1.0e-7 ... 1.2e-7 (1.5e-7 ... 1.7e-7 behind the GELU; 1.8e-7 at the walk test's shape), row sums 0.6e-7 - the bound leaves a factor
5 for the kernel's summation order and its erf polynomial."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from gemm_guarded import NAN, Guarded as _Guarded, Pair as _Pair, PairIL as _PairIL, dev, vec as _vec

pytestmark = pytest.mark.gpu

NO_MEDIUM, ONE_TILE, TILE192, TILE256 = 16, 4, 64, 128
TOL = 1e-6


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import covomix_amd.ops as o
    return o


def _weights(ops, N, K, g):
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev())
    ws = ops.split_f16(w)
    return w, ws, ops.split_f16_interleaved(ws), (ws[0].double() + ws[1].double()) * ws[2]


def _run_all(ops, flags, M, N, K, seed):
    """-> {name: (tensor, ...)} of every output's live region (clones), after the fp64 and guard checks of this tile height"""
    g = torch.Generator().manual_seed(seed)
    parts = N // 64
    x = torch.randn(M, K, generator=g).to(dev())
    a = _PairIL(ops, M, K, x)
    xs = a.value()
    w, ws, wil, wd = _weights(ops, N, K, g)
    b = _vec(N, torch.randn(N, generator=g).to(dev()))
    gamma = _vec(N, (1.0 + 0.3 * torch.randn(N, generator=g)).to(dev()))
    r = _Guarded(M, N, data=torch.randn(M, N, generator=g).to(dev()))
    rs = _vec(M, (0.5 + torch.rand(M, generator=g)).to(dev()))
    cs, hs, sa, sb = (torch.tensor([v], device=dev()) for v in (4.0, 8.0, 2.0, 32.0))
    ref = xs @ wd.T
    bd, rd = b.double(), r.v.double()
    out = {}
    kw = dict(w_split=ws, w_il=wil, a_split=a.il)

    def sums(want):
        return want.square().reshape(M, parts, 64).sum(-1)

    def check(name, want, c=None, pair=None, pair_scale=1.0, rowsq=None, pair_want=None, unwritten=None):
        keep = []
        for what, buf in (("c", c), ("pair", pair), ("rowsq", rowsq)):
            if buf is None:
                continue
            got = buf.value() / pair_scale if what == "pair" else buf.v.double()
            target = sums(want) if what == "rowsq" else (pair_want if what == "pair" and pair_want is not None else want)
            e = rel_l2(got, target)
            print(f"FIGURE {name} M={M} N={N} K={K} flags={flags} {what}: rel-L2 {e:.3e}")
            assert e < TOL, (name, what, flags, e)
            assert buf.guards_untouched(), (name, what, flags)
            keep += [t.clone() for t in (buf.halves() if what == "pair" else (buf.v,))]
        if unwritten is not None:
            assert bool(torch.isnan(unwritten.big).all()), (name, flags)
        assert a.guards_untouched() and r.guards_untouched()
        out[name] = tuple(keep)

    with ops.gemm_flags(flags):
        # res: bias + fp32 residual, fp32 store and a twin
        c, tw = _Guarded(M, N), _Pair(M, N)
        ops.gemm(x, w, c.v, bias=b, residual=r.v, out_split=tw.pair, **kw)
        check("res", ref + bd + rd, c=c, pair=tw)
        # res_tw, fp32 residual: fp32 store, twin * gamma * 4, row sums of squares
        c, tw, q = _Guarded(M, N), _PairIL(ops, M, N), _Guarded(M, parts, pad=4)
        ops.gemm(x, w, c.v, bias=b, residual=r.v, out_split=tw.il, c_scale=cs, c_gamma=gamma, c_rowsq=q.v, **kw)
        want = ref + bd + rd
        check("res_tw", want, c=c, pair=tw, pair_scale=4.0, rowsq=q, pair_want=want * gamma.double())
        # res_tw, the residual as a pair that is also the output pair (the model's residual stream), no fp32 store
        c, rp, q = _Guarded(M, N), _PairIL(ops, M, N, r.v, 8.0), _Guarded(M, parts, pad=4)
        held = rp.value() / 8.0
        ops.gemm(x, w, c.v, bias=b, res_split=rp.il, res_scale=hs, out_split=rp.il, c_scale=hs, c_rowsq=q.v, write_f32=False, **kw)
        check("res_tw_in_place", ref + bd + held, pair=rp, pair_scale=8.0, rowsq=q, unwritten=c)
        # bias_tw: A | A2 with pre-scales 2 and 32
        K1 = K - 32
        a1, a2 = _PairIL(ops, M, K1, x[:, :K1], 2.0), _PairIL(ops, M, 32, x[:, K1:], 32.0)
        xs2 = torch.cat((a1.value() / 2.0, a2.value() / 32.0), 1)
        c, tw, q = _Guarded(M, N), _PairIL(ops, M, N), _Guarded(M, parts, pad=4)
        ops.gemm(x[:, :K1], w, c.v, bias=b, a2=x[:, K1:], w_split=ws, w_il=wil, a_split=a1.il, a2_split=a2.il, a_scale=sa, a2_scale=sb,
                 out_split=tw.il, c_gamma=gamma, c_rowsq=q.v)
        want = xs2 @ wd.T + bd
        check("bias_tw", want, c=c, pair=tw, rowsq=q, pair_want=want * gamma.double())
        assert a1.guards_untouched() and a2.guards_untouched()
        # gelu_split
        c, o = _Guarded(M, N), _Pair(M, N)
        ops.gemm(x, w, c.v, bias=b, act=1, out_split=o.pair, write_f32=False, **kw)
        check("gelu_split", F.gelu(ref + bd), pair=o, unwritten=c)
        # gelu_rs: a factor per row on the accumulators
        c, o = _Guarded(M, N), _PairIL(ops, M, N)
        ops.gemm(x, w, c.v, bias=b, act=1, out_split=o.il, write_f32=False, a_row_scale=rs, **kw)
        check("gelu_rs", F.gelu(ref * rs.double()[:, None] + bd), pair=o, unwritten=c)
        # bias
        c = _Guarded(M, N)
        ops.gemm(x, w, c.v, bias=b, **kw)
        check("bias", ref + bd, c=c)
    return out


@pytest.mark.parametrize("K", [64, 96])
@pytest.mark.parametrize("N", [512, 576])
@pytest.mark.parametrize("M", [2048, 2049, 2303])
def test_row_epilogues_at_tile_edges_in_both_tile_heights(ops, M, N, K):
    seed = M * 7 + N + K
    t256 = _run_all(ops, NO_MEDIUM | TILE256, M, N, K, seed)
    t192 = _run_all(ops, NO_MEDIUM | TILE192, M, N, K, seed)
    assert t256.keys() == t192.keys() and len(t256) == 7
    for name in t256:
        assert len(t256[name]) == len(t192[name]) > 0
        for x256, x192 in zip(t256[name], t192[name]):
            assert torch.equal(x256, x192), (name, M, N, K)


def test_deferred_norm_epilogues_when_a_block_walks_several_tiles(ops):
    """M = 5000 x N = 4096 = 384 tile slots (test_gemm_persistent_blocks_walk_several_tiles): more than one per CU, so a block goes
    through the tile switch with the res_tw (pair residual in place, row sums) and gelu_rs epilogues between its tiles.  Bit-identical to
    one tile per block (CVX_GEMM_FLAG_ONE_TILE), and against fp64."""
    M, N, K = 5000, 4096, 128
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g).to(dev())
    a = _PairIL(ops, M, K, x)
    w, ws, wil, wd = _weights(ops, N, K, g)
    b = torch.randn(N, generator=g).to(dev())
    r = torch.randn(M, N, generator=g).to(dev())
    rs = (0.5 + torch.rand(M, generator=g)).to(dev())
    hs = torch.tensor([8.0], device=dev())
    ref = a.value() @ wd.T
    got = []
    for flags in (NO_MEDIUM, NO_MEDIUM | ONE_TILE):
        with ops.gemm_flags(flags):
            rp, q = _PairIL(ops, M, N, r, 8.0), _Guarded(M, N // 64, pad=4)
            held = rp.value() / 8.0
            dummy = torch.full((M, N), 7.0, device=dev())
            ops.gemm(x, w, dummy, bias=b, w_split=ws, w_il=wil, a_split=a.il, res_split=rp.il, res_scale=hs, out_split=rp.il, c_scale=hs,
                     c_rowsq=q.v, write_f32=False)
            o = _PairIL(ops, M, N)
            ops.gemm(x, w, dummy, bias=b, act=1, w_split=ws, w_il=wil, a_split=a.il, out_split=o.il, write_f32=False, a_row_scale=rs)
            assert bool((dummy == 7.0).all())
            assert rp.guards_untouched() and q.guards_untouched() and o.guards_untouched()
            got.append((rp.v.clone(), q.v.clone(), o.v.clone()))
            if flags == NO_MEDIUM:
                want = ref + b.double() + held
                e = (rel_l2(rp.value() / 8.0, want), rel_l2(q.v.double(), want.square().reshape(M, N // 64, 64).sum(-1)),
                     rel_l2(o.value(), F.gelu(ref * rs.double()[:, None] + b.double())))
                print(f"FIGURE walk res_tw pair {e[0]:.3e}, row sums {e[1]:.3e}, gelu_rs pair {e[2]:.3e}")
                assert max(e) < TOL, e
    for walked, single in zip(*got):
        assert torch.equal(walked, single)
