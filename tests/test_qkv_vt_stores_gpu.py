"""GPU: the V^T stores of a to_qkv GEMM on the eight-phase kernels - line-major, 16 bytes per lane after a half-wave exchange - against
the earlier store code (CVX_GEMM_FLAG_VT_PIECES = 512: 8 bytes per lane, row group by row group) and against fp64.

Only which lane stores which bytes, and in what order, differs: every buffer must come out BIT-IDENTICAL, the untouched bytes (a
sentinel in columns >= T and in the slots of frames that do not exist) included, and the new path keeps the bound of
test_attention_f16x3_with_qkv_transposed_epilogue (rel-L2 < 2e-6 of hi + lo against the fp32 GEMM, read at ops.vt_frame_slots).

The kernels take the operands as interleaved pairs (SplitIL).  N = 3 * H * 64 below 512 columns (H <= 2) runs on the medium-problem
kernel (128 x 128 tiles, two row groups per wave) whatever M is; the large-problem kernel (8 or 6 row groups per wave) needs H >= 3 and
RoPE on whole 256-column groups, so every shape that is to reach a branch of it is run at H = 4 as well, pinned with
CVX_GEMM_FLAG_NO_MEDIUM = 16 (at these row counts the library itself would take the medium kernel)."""
import math

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

NO_MEDIUM, TILE192, TILE256, VT_PIECES = 16, 64, 128, 512
SENTINEL = 777.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import covomix_amd.ops as o
    return o


def dev():
    return torch.device("cuda:0")


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev())


def _rope(positions):
    inv = (1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))).to(dev())
    ang = positions.to(dev()).float()[:, None] * inv[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


class _Problem:
    """x [M, 128], w [3 H 64, 128] and their interleaved pairs, made once per shape"""

    def __init__(self, ops, M, H, seed=140):
        self.M, self.H, self.N = M, H, 3 * H * 64
        self.x = _randn(M, 128, seed=seed)
        self.w = _randn(self.N, 128, seed=seed + 1) / math.sqrt(128) * 1.5
        self.ws = ops.split_f16(self.w)
        self.wil = ops.split_f16_interleaved(self.ws)
        self.il = ops.SplitIL(M, 128, dev())
        ops.split_act_f16(self.x, self.il)

    def run(self, ops, flags, rope, vt_rows, vt_cols, fill=SENTINEL, **kw):
        """-> (qk_hi, qk_lo, vt_hi, vt_lo); every buffer pre-filled, so bytes the launch leaves alone are seen"""
        M, H = self.M, self.H
        qk = tuple(torch.full((M, 2 * H * 64), fill, dtype=torch.float16, device=dev()) for _ in range(2))
        vt = tuple(torch.full((vt_rows, vt_cols), fill, dtype=torch.float16, device=dev()) for _ in range(2))
        with ops.gemm_flags(flags):
            ops.gemm(self.x, self.w, torch.empty(M, self.N, device=dev()), rope=rope, rope_cols=2 * H * 64, w_split=self.ws, w_il=self.wil,
                     a_split=self.il, out_split=qk, vt_split=vt, write_f32=False, **kw)
        torch.cuda.synchronize()
        return qk + vt


def _same(new, old):
    for name, a, b in zip(("qk_hi", "qk_lo", "vt_hi", "vt_lo"), new, old):
        assert torch.equal(a, b), (name, int((a != b).sum()))


def _check_batch(ops, Bt, T, H, flags):
    pb = _Problem(ops, Bt * T, H)
    rope = _rope(torch.arange(T))
    Tp = ((T + 31) // 32) * 32
    new = pb.run(ops, flags, rope, Bt * H * 64, Tp)
    old = pb.run(ops, flags | VT_PIECES, rope, Bt * H * 64, Tp)
    _same(new, old)
    ref = torch.empty(Bt * T, pb.N, device=dev())
    ops.gemm(pb.x, pb.w, ref, rope=rope, rope_cols=2 * H * 64)                        # the fp32 GEMM
    v_ref = ref[:, 2 * H * 64:].reshape(Bt, T, H, 64).permute(0, 2, 3, 1).reshape(Bt * H * 64, T)
    slots = ops.vt_frame_slots(T, dev())
    free = torch.ones(Tp, dtype=torch.bool, device=dev()); free[slots] = False
    v = new[2].float() + new[3].float()
    e_qk, e_v = rel_l2(new[0].float() + new[1].float(), ref[:, : 2 * H * 64]), rel_l2(v[:, slots], v_ref)
    print(f"FIGURE to_qkv Bt={Bt} T={T} H={H} flags={flags}: q|k {e_qk:.3e}, v {e_v:.3e}")
    assert e_qk < 2e-6 and e_v < 2e-6
    assert bool((new[2][:, free] == SENTINEL).all()) and bool((new[3][:, free] == SENTINEL).all())
    return pb, rope, ref


# the shapes as listed (H <= 2: the medium-problem kernel, PRE form, two row groups per wave)
@pytest.mark.parametrize("Bt,T,H,flags", [
    (3, 1000, 2, 0),                      # offsets 0 / 8 / 0 of a slot block, sequence ends inside tiles
    (5, 520, 2, 0),                       # T % 16 = 8
    (9, 260, 2, 0),                       # T % 16 = 4: every sequence but each fourth on the 8-byte stores
    (2, 1030, 2, 0),                      # T % 4 = 2: scalar stores
    (3, 1000, 2, TILE192), (3, 1000, 2, TILE256),
    (2, 136, 2, 0), (1, 1000, 1, 0), (1, 132, 3, 0),          # few rows; H % 4 != 0
])
def test_vt_stores_bit_identical_as_listed(ops, Bt, T, H, flags):
    _check_batch(ops, Bt, T, H, flags)


# the same branches on the large-problem kernel: 2048 rows and more, H = 4, pinned
@pytest.mark.parametrize("Bt,T,flags", [
    (3, 1000, NO_MEDIUM),
    (5, 520, NO_MEDIUM),
    (9, 260, NO_MEDIUM),
    (2, 1030, NO_MEDIUM),
    (3, 1000, NO_MEDIUM | TILE192), (3, 1000, NO_MEDIUM | TILE256),        # 6 / 8 row groups per wave
])
def test_vt_stores_bit_identical_large_kernel(ops, Bt, T, flags):
    _check_batch(ops, Bt, T, 4, flags)


@pytest.mark.parametrize("flags", [0, NO_MEDIUM | TILE192, NO_MEDIUM | TILE256])
def test_vt_stores_deferred_norm_consumer(ops, flags):
    """The consumer form of a deferred norm (a factor per row on the accumulators, plus a bias) re-reads its row factors once per column
    group.  It runs on the large-problem kernel only (the entry point refuses it below 512 columns): H = 4.  Against fp64."""
    Bt, T, H = 3, 1000, 4
    pb = _Problem(ops, Bt * T, H, seed=150)
    rope = _rope(torch.arange(T))
    Tp = ((T + 31) // 32) * 32
    rs = (_randn(Bt * T, seed=152).abs() + 0.25).contiguous()
    bias = _randn(pb.N, seed=153)
    new = pb.run(ops, flags, rope, Bt * H * 64, Tp, a_row_scale=rs, bias=bias)
    old = pb.run(ops, flags | VT_PIECES, rope, Bt * H * 64, Tp, a_row_scale=rs, bias=bias)
    _same(new, old)
    xs = pb.il.dense()[0].double() + pb.il.dense()[1].double()
    z = (xs @ pb.w.double().T) * rs.double()[:, None] + bias.double()
    v_ref = z[:, 2 * H * 64:].reshape(Bt, T, H, 64).permute(0, 2, 3, 1).reshape(Bt * H * 64, T)
    zq = z[:, : 2 * H * 64].reshape(Bt * T, 2 * H, 64)
    c_, s_ = (torch.cat((t, t), -1).double().repeat(Bt, 1)[:, None, :] for t in rope)          # the fp32 tables the kernel reads
    qk_ref = (zq * c_ + torch.cat((-zq[..., 32:], zq[..., :32]), -1) * s_).reshape(Bt * T, -1)
    slots = ops.vt_frame_slots(T, dev())
    e_qk = rel_l2(new[0].double() + new[1].double(), qk_ref)
    e_v = rel_l2((new[2].double() + new[3].double())[:, slots], v_ref)
    print(f"FIGURE to_qkv deferred-norm consumer flags={flags}: q|k {e_qk:.3e}, v {e_v:.3e}")
    assert e_qk < 2e-6 and e_v < 2e-6


@pytest.mark.parametrize("H,flags", [(2, 0), (4, NO_MEDIUM)])
def test_vt_stores_ragged_launch(ops, H, flags):
    """A packed batch: per-row RoPE tables (rope_T = M), one global V^T of M columns - every row group at offset 0 of a slot block."""
    lengths = [1000, 777, 520]
    rg = ops.Ragged(lengths, dev())
    pb = _Problem(ops, rg.M, H, seed=160)
    rope = _rope(rg.positions())
    Mp = (rg.M + 31) // 32 * 32 + 64
    new = pb.run(ops, flags, rope, H * 64, Mp)
    old = pb.run(ops, flags | VT_PIECES, rope, H * 64, Mp)
    _same(new, old)
    ref = torch.empty(rg.M, pb.N, device=dev())
    ops.gemm(pb.x, pb.w, ref, rope=rope, rope_cols=2 * H * 64)
    slots = ops.vt_frame_slots(rg.M, dev())
    free = torch.ones(Mp, dtype=torch.bool, device=dev()); free[slots] = False
    e_v = rel_l2((new[2].float() + new[3].float())[:, slots], ref[:, 2 * H * 64:].T)
    print(f"FIGURE to_qkv ragged H={H}: v {e_v:.3e}")
    assert e_v < 2e-6 and rel_l2(new[0].float() + new[1].float(), ref[:, : 2 * H * 64]) < 2e-6
    assert bool((new[2][:, free] == SENTINEL).all()) and bool((new[3][:, free] == SENTINEL).all())


@pytest.mark.parametrize("H,flags", [(2, 0), (4, NO_MEDIUM)])
def test_attention_on_the_new_vt(ops, H, flags):
    """the V^T of the new stores (zero padding, as the model keeps it) -> split-precision attention, against fp64"""
    Bt, T = 3, 1000
    pb = _Problem(ops, Bt * T, H)
    rope = _rope(torch.arange(T))
    Tp = ((T + 31) // 32) * 32
    qh, ql, vh, vl = pb.run(ops, flags, rope, Bt * H * 64, Tp, fill=0.0)
    ref = torch.empty(Bt * T, pb.N, device=dev())
    ops.gemm(pb.x, pb.w, ref, rope=rope, rope_cols=2 * H * 64)
    out = torch.full((Bt, T, H * 64), float("nan"), device=dev())
    ops.attention_f16x3((qh, ql), (vh, vl), out, Bt, T, H, 0.125)
    q, k, v = ref.double().reshape(Bt, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    want = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).permute(0, 2, 1, 3).reshape(Bt, T, H * 64)
    e = rel_l2(out, want)
    print(f"FIGURE attention on the new V^T H={H}: {e:.3e}")
    assert e < 5e-6
