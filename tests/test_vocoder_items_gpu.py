"""GPU: every vocoder kernel that takes a per-item length table (cvx_item_lengths) against fp64 torch on each item ALONE, with the
items' ends on a tile boundary, one position either side of it, within a convolution's padding of it, at 0, 1, L - 1, L and
through both clamps of the affine length (oracle/vocoder_items_oracle.py: length_launches).  Every case:
  inputs (x / z, res, accum) are zero behind each item's end, biases are >= 0.1 in magnitude, outputs are pre-filled with a
  sentinel on the signal rows (zeros in the halos);
  (a) exact zeros behind every item's end, in the halos and in the padded channels;
  (b) items of full length are bit-equal to the launch without a table (same shape, same stream);
  (c) rel-L2 over all valid positions within the bound of the kernel's test without a table (+ max-abs where that test has it);
  (d) per item, rel-L2 over its last min(32, n_b) valid positions <= 4 x that bound.
tests/test_vocoder_items_oracle.py proves on the pair / ResBlock inputs used here that (a) and (d) catch an unmasked intermediate,
an end that is off by one and an accumulate behind the end.  Tile forms and persistent grids are steered with the launch context's
CU count (no CU mask); the form is asserted through the library's own rule (ops.hifigan_conv1d_form)."""
import contextlib
from types import SimpleNamespace

import pytest
import torch

import vocoder_items_oracle as vio

pytestmark = pytest.mark.gpu

from covomix_amd import ops  # noqa: E402

H = ops.HIFI_HALO_L
SENT = 1.5
DEV = torch.device("cuda:0")


@contextlib.contextmanager
def small_cus(n):
    """run on a plain stream whose launch context says it owns n CUs (n = 0: the device's); the context is restored afterwards -
    torch hands stream handles out of a pool, so a later test may meet the same one"""
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ctx = ops.ctx_of(st)
    before = ctx.n_cus
    if n:
        ctx.n_cus = n
    try:
        with torch.cuda.stream(st):
            yield st
            st.synchronize()
    finally:
        ctx.n_cus = before
        torch.cuda.synchronize()


def np_of(c):
    return 32 if c <= 32 else 64 if c <= 64 else 128 if c <= 128 else 256


def to_cl(x, np_, z=False, scale=None):
    """[B, C, L] fp32 on the GPU -> zero-haloed channels-last fp32 copy, or (z) the split pair of leaky_relu(x) * scale"""
    B, _, L = x.shape
    Lp = ops.hifigan_cl_rows(L)
    if z:
        pair = (torch.zeros(B, Lp, np_, dtype=torch.float16, device=DEV), torch.zeros(B, Lp, np_, dtype=torch.float16, device=DEV))
        ops.hifigan_to_channels_last(x.contiguous(), None, pair, 0.1, z_scale=scale)
        return pair
    buf = torch.zeros(B, Lp, np_, device=DEV)
    ops.hifigan_to_channels_last(x.contiguous(), buf, None, 1.0)
    return buf


def sentinel(B, L, np_, dtype=torch.float32):
    buf = torch.zeros(B, ops.hifigan_cl_rows(L), np_, dtype=dtype, device=DEV)
    buf[:, H:H + L] = SENT
    return buf


def view(buf, C, L):
    return buf[:, H:H + L, :C].transpose(1, 2)


def outside_max(buf, C, lens):
    """(a) on a channels-last buffer: the largest magnitude outside rows [H, H + n_b) x channels [0, C)"""
    m = buf.float().abs().clone()
    for b, n in enumerate(lens):
        m[b, H:H + n, :C] = 0
    return float(m.max())


def scale_of(x):
    s = torch.ones(1, device=DEV)
    ops.amax_pow2_scale(x.contiguous(), 1024.0, s, torch.zeros(1, dtype=torch.int32, device=DEV))
    return s


def items_of(launch):
    frames, mul, add = launch
    return (torch.tensor(frames, dtype=torch.int32, device=DEV), mul, add)


def check(label, got, want, lens, bound, maxabs=False):
    """(a) on the [B, C, L] view, (c) and (d); prints every figure before it asserts"""
    behind = vio.max_behind(got, lens)
    c = vio.rel_valid(got, want, lens)
    d = max(vio.rel_tails(got, want, lens))
    ma = max(float((got[b, :, :n].double() - want[b, :, :n]).abs().max()) for b, n in enumerate(lens) if n > 0) / float(want.abs().max())
    print(f"{label}: (a) {behind:.1e}  (c) {c:.3e} / {bound:.0e}  (d) {d:.3e} / {4 * bound:.0e}  max-abs {ma:.3e}")
    assert behind == 0.0, label
    assert c < bound, (label, c)
    assert d <= 4 * bound, (label, d)
    if maxabs:
        assert ma < 1e-5, (label, ma)
    return c, d


def full_items_equal(lens, L, got, base):
    return all(torch.equal(got[b], base[b]) for b, n in enumerate(lens) if n == L)


def conv_ns(c, k, dil, np_):
    """(w, b) fp32 on the GPU -> the object the ResBlock front ends take"""
    o = SimpleNamespace(k=k, dil=dil, w16=ops.hifigan_pack_weight_f16x3(c[0]))
    o.bias16 = torch.zeros(np_, device=DEV)
    o.bias16[:c[1].numel()] = c[1]
    return o


def dev2(c):
    return c[0].to(DEV), c[1].to(DEV)


# ---------------------------------------------------------------- cvx_hifigan_conv1d_f16x3
CONV_SHAPES = [(31, 601, 256), (62, 601, 256), (125, 601, 256), (250, 320, 160), (250, 384, 192), (250, 512, 256)]


@pytest.mark.parametrize("k,dil", vio.PAIR_KD)
@pytest.mark.parametrize("C,L,R", CONV_SHAPES)
def test_conv1d_f16x3_items(C, L, R, k, dil):
    """Np = 32 / 64 / 128 (256-row tiles) and Np = 256 in its three tile forms (contexts of 2 B CUs: 160 rows at L = 320, 192 at
    384, 256 at 512), with res, accum, out_scale, out_x and out_z."""
    pad, np_ = (k - 1) * dil // 2, np_of(C)
    g = torch.Generator().manual_seed(C * 100 + k)
    w, b = dev2(vio.conv_weights(g, C, k))
    wpk = ops.hifigan_pack_weight_f16x3(w)
    bias = torch.zeros(np_, device=DEV)
    bias[:C] = b
    for li, la in enumerate(vio.length_launches(R, pad, L)):
        lens, B = vio.lens_of(la, L), len(la[0])
        with small_cus(2 * B):
            assert ops.hifigan_conv1d_form(np_, L, B) == R
            x, res, acc = (vio.zero_tails(vio.randn(g, B, C, L), lens).to(DEV) for _ in range(3))
            z, res_cl, acc_cl = to_cl(x, np_, z=True), to_cl(res, np_), to_cl(acc, np_)
            outs = []
            for items in (items_of(la), None):
                ox = sentinel(B, L, np_)
                oz = (sentinel(B, L, np_, torch.float16), sentinel(B, L, np_, torch.float16))
                ops.hifigan_conv1d_f16x3(z, wpk, bias, B, L, ksize=k, dil=dil, res=res_cl, accum=acc_cl, out_x=ox, out_scale=1.0 / 3,
                                         out_z=oz, z_slope=0.1, items=items)
                outs.append((ox, oz))
            (ox, oz), (bx, bz) = outs
            want = [vio.per_item(lambda b_, n, xb, rb, ab, j=j: vio.conv_item(xb, w.double(), b.double(), dil, rb, ab, 1.0 / 3)[j],
                                 lens, L, C, x, x, res, acc) for j in (0, 1)]
            for t in (ox, oz[0], oz[1]):
                assert outside_max(t, C, lens) == 0.0
            assert full_items_equal(lens, L, ox, bx) and full_items_equal(lens, L, oz[0], bz[0]) and full_items_equal(lens, L, oz[1], bz[1])
            check(f"conv1d_f16x3 C={C} k={k} form={R} launch {li} out_x", view(ox, C, L), want[0], lens, 2e-6, maxabs=True)
            check(f"conv1d_f16x3 C={C} k={k} form={R} launch {li} out_z", view(oz[0].float() + oz[1].float(), C, L), want[1], lens, 2e-6,
                  maxabs=True)


def test_conv1d_group_f16x3_items():
    """n = 3 (k = 3 / 7 / 11) with a length table: bit-equal to three single calls; members with different tables are refused."""
    from covomix_amd import _lib
    C, L, R, np_ = 125, 601, 256, 128
    la = vio.length_launches(R, 5, L)[1]
    lens, B = vio.lens_of(la, L), len(la[0])
    g = torch.Generator().manual_seed(5)
    x = vio.zero_tails(vio.randn(g, B, C, L), lens).to(DEV)
    z = to_cl(x, np_, z=True)
    items = items_of(la)
    probs, singles = [], []
    for k, dil in vio.PAIR_KD:
        w, b = dev2(vio.conv_weights(g, C, k))
        bias = torch.zeros(np_, device=DEV)
        bias[:C] = b
        pr = dict(z=z, wpk=ops.hifigan_pack_weight_f16x3(w), bias=bias, ksize=k, dil=dil, items=items)
        probs.append(dict(pr, out_x=sentinel(B, L, np_), out_z=(sentinel(B, L, np_, torch.float16), sentinel(B, L, np_, torch.float16))))
        singles.append(dict(pr, out_x=sentinel(B, L, np_), out_z=(sentinel(B, L, np_, torch.float16), sentinel(B, L, np_, torch.float16))))
    ops.hifigan_conv1d_group_f16x3(probs, B, L)
    for pr, sg in zip(probs, singles):
        kw = {key: v for key, v in sg.items() if key not in ("z", "wpk", "bias")}
        ops.hifigan_conv1d_f16x3(sg["z"], sg["wpk"], sg["bias"], B, L, **kw)
        assert torch.equal(pr["out_x"], sg["out_x"]) and torch.equal(pr["out_z"][0], sg["out_z"][0]) and torch.equal(pr["out_z"][1], sg["out_z"][1])
        assert outside_max(pr["out_x"], C, lens) == 0.0 and outside_max(pr["out_z"][0], C, lens) == 0.0
    other = (items[0].clone(), items[1], items[2])                    # the same lengths in ANOTHER table: refused
    with pytest.raises(_lib.CovomixHipError):
        ops.hifigan_conv1d_group_f16x3([probs[0], dict(probs[1], items=other), probs[2]], B, L)
    with pytest.raises(_lib.CovomixHipError):
        ops.hifigan_conv1d_group_f16x3([probs[0], dict(probs[1], items=(items[0], items[1], items[2] - 1)), probs[2]], B, L)


# ---------------------------------------------------------------- cvx_hifigan_resblock_pair_f16x3
@pytest.mark.parametrize("k,dil", vio.PAIR_KD)
@pytest.mark.parametrize("C,flags", vio.PAIR_INST)
def test_resblock_pair_f16x3_items(C, flags, k, dil):
    """The three instantiations on a context of 2 CUs: 2 or 4 persistent blocks walk the 4 tiles of each of up to 8 items, so a
    block goes from one item into the next with the next tile's rows already in flight.  With accum (apart and aliasing out), without,
    and with an accum that breaks the input rule (the kernel zeroes after the accumulate: out is zero behind the end regardless);
    every item bit-equal to its own B = 1, L = n_b launch."""
    R, pad, L, launches = vio.pair_case(C, flags, k, dil)
    np_ = np_of(C)
    c1 = c2 = None
    for li, la in enumerate(launches):
        lens, B = vio.lens_of(la, L), len(la[0])
        x, acc, w1, w2 = vio.pair_inputs(C, k, dil, L, lens, seed=1000 * C + 10 * k + li)
        dirty = vio.dirty_accum(acc, lens, seed=li)
        w1, w2 = dev2(w1), dev2(w2)
        c1, c2 = conv_ns(w1, k, dil, np_), conv_ns(w2, k, 1, np_)
        with small_cus(2):
            x, acc, dirty = x.to(DEV), acc.to(DEV), dirty.to(DEV)
            zs = scale_of(x)
            x_cl, acc_cl, dirty_cl = to_cl(x, np_), to_cl(acc, np_), to_cl(dirty, np_)
            items = items_of(la)
            run = lambda out, **kw: ops.hifigan_resblock_pair_f16x3(x_cl, c1, c2, B, L, out, z_scale=zs, flags=flags, **kw)
            o_acc, o_base, o_plain, o_dirty, o_alias = sentinel(B, L, np_), sentinel(B, L, np_), sentinel(B, L, np_), sentinel(B, L, np_), acc_cl.clone()
            run(o_acc, accum=acc_cl, out_scale=0.5, items=items)
            run(o_base, accum=acc_cl, out_scale=0.5)
            run(o_plain, items=items)
            run(o_dirty, accum=dirty_cl, out_scale=0.5, items=items)
            run(o_alias, accum=o_alias, out_scale=0.5, items=items)
            for t in (o_acc, o_plain, o_dirty, o_alias):
                assert outside_max(t, C, lens) == 0.0
            assert torch.equal(o_alias, o_acc) and torch.equal(o_dirty, o_acc)
            assert full_items_equal(lens, L, o_acc, o_base)
            want = vio.per_item(lambda b_, n, xb, ab: vio.pair_item(xb, vio.dbl(w1), vio.dbl(w2), dil, ab, 0.5), lens, L, C, x, x, acc)
            check(f"pair C={C} flags={flags} k={k} launch {li} accum", view(o_acc, C, L), want, lens, 5e-6)
            want = vio.per_item(lambda b_, n, xb: vio.pair_item(xb, vio.dbl(w1), vio.dbl(w2), dil), lens, L, C, x, x)
            check(f"pair C={C} flags={flags} k={k} launch {li} plain", view(o_plain, C, L), want, lens, 5e-6)
            for b, n in enumerate(lens):                               # its own B = 1, L = n_b launch: same instantiation, same tile origin
                if n == 0:
                    continue
                o1 = sentinel(1, L, np_)
                ops.hifigan_resblock_pair_f16x3(x_cl[b:b + 1].contiguous(), c1, c2, 1, n, o1, accum=acc_cl[b:b + 1].contiguous(), out_scale=0.5,
                                                z_scale=zs, flags=flags)
                assert torch.equal(o1[0, H:H + n], o_acc[b, H:H + n]), (b, n)


# ---------------------------------------------------------------- cvx_hifigan_resblock_f16x3 / _stage_
@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_resblock_stage_f16x3_items(name):
    """One narrow stage (C = 62: fused pair kernels, context of 2 CUs) and one wide stage (C = 125: grouped split convolutions):
    the stage call bit-equal to block after block, both against fp64 per item; on the narrow stage one ResBlock with an accum that
    breaks the input rule."""
    cs = vio.STAGE_CASES[name]
    C, L, np_ = cs["C"], cs["L"], np_of(cs["C"])
    for li, la in enumerate(vio.length_launches(cs["R"], cs["pad"], L)):
        lens, B = vio.lens_of(la, L), len(la[0])
        x, acc, blocks = vio.resblock_inputs(C, vio.STAGE_KS, L, lens, seed=77 + C)
        blocks = [[(dev2(p1), dev2(p2)) for p1, p2 in blk] for blk in blocks]
        with small_cus(2 if name == "narrow" else 0):
            x = x.to(DEV)
            zs = scale_of(x)
            x_cl = to_cl(x, np_)
            z = to_cl(x, np_, z=True, scale=zs) if name == "wide" else None
            nsb = [[(conv_ns(p1, k, vio.RESBLOCK_DILS[m], np_), conv_ns(p2, k, 1, np_)) for m, (p1, p2) in enumerate(blk)]
                   for k, blk in zip(vio.STAGE_KS, blocks)]
            Lp = x_cl.shape[1]
            f32 = lambda: torch.zeros(B, Lp, np_, device=DEV)
            f16 = lambda: (torch.zeros(B, Lp, np_, dtype=torch.float16, device=DEV), torch.zeros(B, Lp, np_, dtype=torch.float16, device=DEV))
            scr = [dict(t=f16(), rz0=f16(), rz1=f16(), r0=f32(), r1=f32()) for _ in nsb]
            items = items_of(la)
            o_stage, o_base, o_seq = sentinel(B, L, np_), sentinel(B, L, np_), sentinel(B, L, np_)
            ops.hifigan_resblock_stage_f16x3(x_cl, z, nsb, B, L, scr, o_stage, out_scale=1.0 / 3, z_scale=zs, items=items)
            for j, blk in enumerate(nsb):
                ops.hifigan_resblock_f16x3(x_cl, z, blk, B, L, scr[j], accum=o_seq if j else None, out=o_seq,
                                           out_scale=1.0 / 3 if j == 2 else 1.0, z_scale=zs, items=items)
            ops.hifigan_resblock_stage_f16x3(x_cl, z, nsb, B, L, scr, o_base, out_scale=1.0 / 3, z_scale=zs)
            assert torch.equal(o_stage, o_seq)
            assert outside_max(o_stage, C, lens) == 0.0
            assert full_items_equal(lens, L, o_stage, o_base)
            want = vio.per_item(lambda b_, n, xb: vio.stage_item(xb, blocks), lens, L, C, x, x)
            check(f"resblock stage {name} launch {li}", view(o_stage, C, L), want, lens, 5e-6)
            if name == "narrow" and li == 1:
                acc = acc.to(DEV)
                dirty = vio.dirty_accum(acc.cpu(), lens, seed=3).to(DEV)
                o_a, o_d = sentinel(B, L, np_), sentinel(B, L, np_)
                ops.hifigan_resblock_f16x3(x_cl, z, nsb[1], B, L, scr[1], accum=to_cl(acc, np_), out=o_a, out_scale=1.0 / 3, z_scale=zs, items=items)
                ops.hifigan_resblock_f16x3(x_cl, z, nsb[1], B, L, scr[1], accum=to_cl(dirty, np_), out=o_d, out_scale=1.0 / 3, z_scale=zs, items=items)
                assert outside_max(o_d, C, lens) == 0.0 and torch.equal(o_d, o_a)
                blk64 = [(vio.dbl(p1), vio.dbl(p2)) for p1, p2 in blocks[1]]
                want = vio.per_item(lambda b_, n, xb, ab: vio.resblock_item(xb, blk64, vio.RESBLOCK_DILS, ab, 1.0 / 3), lens, L, C, x, x, acc)
                check("resblock narrow k=7 accum", view(o_a, C, L), want, lens, 5e-6)


# ---------------------------------------------------------------- the conv-transposes
def convt_inputs(g, B, Cin, L_in, lens, k, u, p):
    """x [B, Cin, L_in] with zeros behind the fewest input positions that give an item its n_b outputs"""
    n_in = [vio.conv_transpose_n_in(n, k, u, p, L_in) for n in lens]
    return vio.zero_tails(vio.randn(g, B, Cin, L_in), n_in), n_in


def convt_want(x, n_in, lens, w, b, u, p, L_out):
    want = torch.zeros(len(lens), w.shape[1], L_out, dtype=torch.float64, device=x.device)
    for i, (n, ni) in enumerate(zip(lens, n_in)):
        if n > 0:
            want[i, :, :n] = vio.conv_transpose_item(x[i, :, :ni].double(), w.double(), b.double(), u, p, n)
    return want


@pytest.mark.parametrize("Cin,Cout,k,u,L_in", [(500, 250, 8, 5, 200), (250, 125, 8, 4, 260)])
def test_conv_transpose1d_f16x3_items(Cin, Cout, k, u, L_in):
    """The first upsampler of config_covomix (L_out = 5 L + 1) and the stride-4 one, lengths in OUTPUT positions; a context of 10 B CUs
    puts both on two 160-row tiles per item (R = 160 * stride outputs; 2 R - pad does not fit into L_out <= 1100).  The fused
    max|out| is the maximum over valid positions only: equal to the output's own maximum, and zero for a launch of empty items."""
    p = (k - u) // 2
    L_out = (L_in - 1) * u + k - 2 * p
    g = torch.Generator().manual_seed(Cin + k)
    w = (vio.randn(g, Cin, Cout, k) / (Cin * k / u) ** 0.5).to(DEV)
    b = vio.bias_of(g, Cout).to(DEV)
    pk = ops.hifigan_pack_conv_transpose1d_f16x3(w, b, u, p)
    nt, M = len(pk["taps"]), -(-L_out // u)
    rows = ops.hifigan_conv1d_form(pk["tile_np"], M, 8, nt, 80)
    assert rows == 160 and M > rows
    launches = vio.length_launches(rows * u, k - 1 - p, L_out) + [([0, 1], 2, -3)]         # the last: every item empty
    for li, la in enumerate(launches):
        lens, B = vio.lens_of(la, L_out), len(la[0])
        with small_cus(10 * B):
            assert ops.hifigan_conv1d_form(pk["tile_np"], M, B, nt) == rows
            x, n_in = convt_inputs(g, B, Cin, L_in, lens, k, u, p)
            x = x.to(DEV)
            zs = scale_of(x) if float(x.abs().max()) > 0 else None
            z = to_cl(x, pk["cp_in"], z=True, scale=zs)
            out, base = sentinel(B, L_out, pk["np_out"]), sentinel(B, L_out, pk["np_out"])
            amax, amax0 = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.hifigan_conv_transpose1d_f16x3(z, pk, B, L_in, out, L_out, z_scale=zs, amax_bits=amax, items=items_of(la))
            ops.hifigan_conv_transpose1d_f16x3(z, pk, B, L_in, base, L_out, z_scale=zs, amax_bits=amax0)
            assert outside_max(out, Cout, lens) == 0.0
            assert full_items_equal(lens, L_out, out, base)
            assert float(amax.view(torch.float32)) == float(out.abs().max())
            if max(lens) == 0:
                assert int(amax) == 0 and float(amax0.view(torch.float32)) >= 0.1          # (the launch without a table sees the bias)
                continue
            want = convt_want(x, n_in, lens, w, b, u, p, L_out)
            check(f"conv_transpose1d_f16x3 {Cin}->{Cout} launch {li}", view(out, Cout, L_out), want, lens, 2e-6, maxabs=True)


def test_conv1d_and_conv_transpose1d_f32_items():
    """cvx_hifigan_conv1d_f32 (up = 1 with res / accum / out_scale; up = 2, the zero-stuffed upsampler) and
    cvx_hifigan_conv_transpose1d_f32 (polyphase, with the fused max|out|): channel-major tensors, 256 outputs (256 inputs per phase:
    512 outputs) per block."""
    g = torch.Generator().manual_seed(9)
    C, k, dil, L = 62, 7, 3, 601
    w, b = dev2(vio.conv_weights(g, C, k))
    wp = ops.hifigan_pack_weight(w, False).to(DEV)
    for li, la in enumerate(vio.length_launches(256, (k - 1) * dil // 2, L)):
        lens, B = vio.lens_of(la, L), len(la[0])
        x, res, acc = (vio.zero_tails(vio.randn(g, B, C, L), lens).to(DEV) for _ in range(3))
        out, base = torch.full((B, C, L), SENT, device=DEV), torch.full((B, C, L), SENT, device=DEV)
        kw = dict(cout=C, ksize=k, dil=dil, pad=(k - 1) * dil // 2, in_slope=0.1, res=res, accum=acc, out_scale=1.0 / 3)
        ops.hifigan_conv1d(x, wp, b, out, items=items_of(la), **kw)
        ops.hifigan_conv1d(x, wp, b, base, **kw)
        assert full_items_equal(lens, L, out, base)
        want = vio.per_item(lambda b_, n, xb, rb, ab: vio.conv_item(xb, w.double(), b.double(), dil, rb, ab, 1.0 / 3)[0], lens, L, C, x, x, res, acc)
        check(f"conv1d_f32 launch {li}", out, want, lens, 2e-6)
    Cin, Cout, k, u, L_in = 62, 31, 4, 2, 300
    p = (k - u) // 2
    L_out = (L_in - 1) * u + k - 2 * p
    w = (vio.randn(g, Cin, Cout, k) / (Cin * k / u) ** 0.5).to(DEV)
    b = vio.bias_of(g, Cout).to(DEV)
    wz, wph = ops.hifigan_pack_weight(w, True).to(DEV), ops.hifigan_pack_conv_transpose1d(w, u, p).to(DEV)
    for name, R in (("zero-stuffed", 256), ("polyphase", 256 * u)):
        launches = vio.length_launches(R, k - 1 - p, L_out) + ([([0, 1], 2, -3)] if name == "polyphase" else [])
        for li, la in enumerate(launches):
            lens, B = vio.lens_of(la, L_out), len(la[0])
            x, n_in = convt_inputs(g, B, Cin, L_in, lens, k, u, p)
            x = x.to(DEV)
            out, base = torch.full((B, Cout, L_out), SENT, device=DEV), torch.full((B, Cout, L_out), SENT, device=DEV)
            if name == "zero-stuffed":
                kw = dict(cout=Cout, ksize=k, dil=1, pad=k - 1 - p, up=u, in_slope=0.1)
                ops.hifigan_conv1d(x, wz, b, out, items=items_of(la), **kw)
                ops.hifigan_conv1d(x, wz, b, base, **kw)
            else:
                amax = torch.zeros(1, dtype=torch.int32, device=DEV)
                kw = dict(cout=Cout, ksize=k, stride=u, padding=p, in_slope=0.1)
                ops.hifigan_conv_transpose1d(x, wph, b, out, amax_bits=amax, items=items_of(la), **kw)
                ops.hifigan_conv_transpose1d(x, wph, b, base, **kw)
                assert float(amax.view(torch.float32)) == float(out.abs().max())
                if max(lens) == 0:
                    assert int(amax) == 0 and float(out.abs().max()) == 0.0 and float(base.abs().max()) >= 0.1
                    continue
            assert full_items_equal(lens, L_out, out, base)
            want = convt_want(x, n_in, lens, w, b, u, p, L_out)
            check(f"conv_transpose f32 {name} launch {li}", out, want, lens, 2e-6)
