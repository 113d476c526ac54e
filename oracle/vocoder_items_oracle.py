"""fp64 oracle of the vocoder kernels' per-item lengths (cvx_item_lengths, include/covomix_hip.h): what a kernel given a length
table must produce is what a B = 1 run of every item ALONE produces (covomix/vocoder/models.py:35-42, :85-88, :100-110 on
x[b, :, :n_b]), placed at [0, n_b) of a zero tensor.  tests/test_vocoder_items_gpu.py compares the HIP kernels with it;
tests/test_vocoder_items_oracle.py proves on the same inputs that the comparison can fail: the `fault` argument of the padded-batch
restatements below builds three deliberately wrong variants.  Plain torch, any device, no project code."""
import torch
import torch.nn.functional as F

SLOPE = 0.1
TAIL = 32               # check (d) looks at an item's last min(TAIL, n_b) valid positions
FAULTS = ("t_unmasked", "len+1", "len-1", "accum_behind")


def item_len(frames: int, mul: int, add: int, L: int) -> int:
    """cvx_item_len: min(L, max(0, frames * mul + add))"""
    return min(L, max(0, frames * mul + add))


def length_launches(R: int, pad: int, L: int):
    """The item lengths one kernel is tested at, through its tile height R and padding pad: 0, 1, R - 1, R, R + 1, R + pad - 1,
    2R - pad (where it fits into L), L - 1, L, one affine value below zero and one above L - as [(frames, mul, add)], two launches of
    at most 8 items; the second has mul = 2 and add < 0 (its targets share the parity of R + pad - 1)."""
    assert 1 <= pad < R and R + pad - 1 <= L - 1 and R + 1 < L - 1
    first = [L, 0, 1, R - 1, R, R + 1, L - 1]
    if 2 * R - pad <= L:
        first.append(2 * R - pad)
    t1 = R + pad - 1
    add = -3 if t1 % 2 else -4
    same = [t for t in (R - 1, R, R + 1, L - 1, L) if t % 2 == t1 % 2 and t != t1][0]
    second = [(t1 - add) // 2, 1, L, (same - add) // 2]          # frames 1 -> 2 + add < 0 (clamped to 0); frames L -> above L (clamped)
    assert 2 + add < 0 and 2 * L + add > L
    return [(first, 1, 0), (second, 2, add)]


def lens_of(launch, L: int):
    frames, mul, add = launch
    return [item_len(f, mul, add, L) for f in frames]


def required_lengths(R: int, pad: int, L: int):
    return {0, 1, R - 1, R, R + 1, R + pad - 1, L - 1, L} | ({2 * R - pad} if 2 * R - pad <= L else set())


def lrelu(x):
    return F.leaky_relu(x, SLOPE)


def zero_tails(x, lens):
    """the header's input rule: zeros behind every item's end (x: [B, C, L], a copy is returned)"""
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, :, n:] = 0
    return x


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def bias_of(g, C):
    """|bias| >= 0.1 in every channel: an intermediate that should have been masked is far from zero"""
    r = randn(g, C)
    return torch.where(r >= 0, 0.1 + 0.1 * r.abs(), -0.1 - 0.1 * r.abs())


def conv_weights(g, C, k, cout=None):
    cout = cout or C
    return randn(g, cout, C, k) / (C * k) ** 0.5, bias_of(g, cout)


# ---------------------------------------------------------------- per item, B = 1: the expected values
def _same(x, w, b, dil):
    return F.conv1d(x[None], w, b, dilation=dil, padding=(w.shape[2] - 1) * dil // 2)[0]


def conv_item(x, w, b, dil, res=None, accum=None, out_scale=1.0):
    """one convolution of cvx_conv16_args / cvx_conv_args (up = 1) on x [C, n]: (out_x, out_z)"""
    v = _same(lrelu(x), w, b, dil)
    if res is not None:
        v = v + res
    return ((v + accum) if accum is not None else v) * out_scale, lrelu(v)


def pair_item(x, c1, c2, dil, accum=None, out_scale=1.0):
    """models.py:36-40: c2(lrelu(c1(lrelu(x)))) + x (+ accum), scaled"""
    y = _same(lrelu(_same(lrelu(x), c1[0], c1[1], dil)), c2[0], c2[1], 1) + x
    return ((y + accum) if accum is not None else y) * out_scale


def resblock_item(x, block, dils, accum=None, out_scale=1.0):
    """ResBlock1.forward, models.py:35-42; block = [(c1, c2)] * 3, c = (w, b)"""
    y = x
    for m in range(3):
        y = pair_item(y, block[m][0], block[m][1], dils[m])
    return ((y + accum) if accum is not None else y) * out_scale


def conv_transpose_item(x, w, b, stride, padding, n_out):
    """leaky_relu + ConvTranspose1d (models.py:102-103) of x [Cin, n_in], its first n_out outputs"""
    return F.conv_transpose1d(lrelu(x)[None], w, b, stride=stride, padding=padding)[0][:, :n_out]


def conv_transpose_n_in(n_out, k, stride, padding, L_in):
    """fewest input positions whose transposed convolution has n_out outputs or more (0 for none)"""
    if n_out <= 0:
        return 0
    return min(L_in, max(1, -(-(n_out - (k - 2 * padding)) // stride) + 1))


def per_item(fn, lens, L, C_out, like, *tensors):
    """out[b, :, :n_b] = fn(b, n_b, *[t[b, :, :n_b]]) for every item with n_b > 0; zeros elsewhere.  tensors: [B, C, L] or None"""
    out = torch.zeros(len(lens), C_out, L, dtype=torch.float64, device=like.device)
    for b, n in enumerate(lens):
        if n > 0:
            out[b, :, :n] = fn(b, n, *[None if t is None else t[b, :, :n].double() for t in tensors])
    return out


# ---------------------------------------------------------------- the padded-batch restatement, with faults
def _nm(n, L, fault):
    return min(L, max(0, n + (1 if fault == "len+1" else -1 if fault == "len-1" else 0)))


def pair_padded(x, n, c1, c2, dil, accum=None, out_scale=1.0, fault=None):
    """What the fused pair kernel computes for ONE item of a ragged launch, on the item's whole row x [C, L] (zeros behind n):
    fault None equals pair_item on x[:, :n].  Faults: 't_unmasked' - the intermediate is not zeroed behind the item's end;
    'len+1' / 'len-1' - the end is off by one; 'accum_behind' - accum is added behind the end (after the zeroing)."""
    assert fault is None or fault in FAULTS
    L = x.shape[1]
    nm = _nm(n, L, fault)
    t = lrelu(_same(lrelu(x), c1[0], c1[1], dil))
    if fault != "t_unmasked":
        t[:, nm:] = 0
    y = _same(t, c2[0], c2[1], 1) + x
    if accum is not None and fault != "accum_behind":
        y = y + accum
    y[:, nm:] = 0
    if accum is not None and fault == "accum_behind":
        y = y + accum
    return y * out_scale


def resblock_padded(x, n, block, dils, accum=None, out_scale=1.0, fault=None):
    y = x
    for m in range(3):
        last = m == 2
        y = pair_padded(y, n, block[m][0], block[m][1], dils[m], accum if last else None, out_scale if last else 1.0, fault)
    return y


# ---------------------------------------------------------------- the checks both test files apply
def max_behind(out, lens):
    """check (a) on a [B, C, L] tensor: the largest magnitude behind an item's end (must be exactly 0)"""
    m = 0.0
    for b, n in enumerate(lens):
        if n < out.shape[2]:
            m = max(m, float(out[b, :, n:].abs().max()))
    return m


def rel_valid(out, want, lens):
    """check (c): rel-L2 over all valid positions of the batch"""
    num = sum(float((out[b, :, :n].double() - want[b, :, :n]).pow(2).sum()) for b, n in enumerate(lens))
    den = sum(float(want[b, :, :n].pow(2).sum()) for b, n in enumerate(lens))
    return (num / max(den, 1e-300)) ** 0.5


def rel_tails(out, want, lens):
    """check (d): per item with n_b > 0, rel-L2 over its last min(32, n_b) valid positions"""
    r = []
    for b, n in enumerate(lens):
        if n > 0:
            s = slice(max(0, n - TAIL), n)
            r.append(float((out[b, :, s].double() - want[b, :, s]).norm() / want[b, :, s].norm().clamp_min(1e-300)))
    return r


# ---------------------------------------------------------------- the inputs of the pair / ResBlock cases (shared: GPU test and proof)
PAIR_KD = ((3, 1), (7, 3), (11, 5))
PAIR_INST = ((31, 0), (62, 0), (62, 1))             # (channels, flags): Np = 32, Np = 64, Np = 64 on 128-row tiles
RESBLOCK_DILS = (1, 3, 5)


def pair_rows(C, flags):
    return 128 if (C > 32 and flags & 1) else 256


def pair_case(C, flags, k, dil):
    """R = the kernel's output tile (rows - (k - 1)), pad = conv2's padding (its last pad outputs read the intermediate behind
    the end), L = 3 R + 17: four tiles per item, so two blocks walk from one item into the next"""
    R, pad = pair_rows(C, flags) - (k - 1), (k - 1) // 2
    L = 3 * R + 17
    return R, pad, L, length_launches(R, pad, L)


def pair_inputs(C, k, dil, L, lens, seed):
    """x, accum (zero behind the ends), c1, c2 - fp32, CPU"""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    x, acc = zero_tails(randn(g, B, C, L), lens), zero_tails(randn(g, B, C, L), lens)
    return x, acc, conv_weights(g, C, k), conv_weights(g, C, k)


def dirty_accum(acc, lens, seed):
    """an accum that BREAKS the input rule (non-zero behind the ends): the launch that pins 'zero behind the end whatever accum holds'"""
    g = torch.Generator().manual_seed(seed + 7)
    d = acc.clone()
    for b, n in enumerate(lens):
        d[b, :, n:] = randn(g, acc.shape[1], acc.shape[2] - n) + 2.0
    return d


def resblock_inputs(C, ks, L, lens, seed):
    """x, accum and one block (3 x (c1, c2)) per kernel size of ks"""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    x, acc = zero_tails(randn(g, B, C, L), lens), zero_tails(randn(g, B, C, L), lens)
    blocks = [[(conv_weights(g, C, k), conv_weights(g, C, k)) for _ in range(3)] for k in ks]
    return x, acc, blocks


def dbl(c):
    """weights (w, b) -> fp64"""
    return c[0].double(), c[1].double()


# one generator stage (models.py:104-110): xs = sum_j resblocks[j](x) / num_kernels, kernel sizes 3 / 7 / 11
STAGE_KS = (3, 7, 11)
STAGE_CASES = {"narrow": dict(C=62, R=256 - 10, pad=5, L=3 * 246 + 17),        # fused pair kernels; R: the k = 11 block's output tile
               "wide": dict(C=125, R=256, pad=5, L=601)}                        # split convolutions, 256-row tiles


def stage_item(x, blocks):
    return sum(resblock_item(x, [(dbl(c1), dbl(c2)) for c1, c2 in blk], RESBLOCK_DILS) for blk in blocks) / len(blocks)


def stage_padded(x, n, blocks, fault=None, faulty_blocks=None):
    """the stage on an item's whole row; the fault sits in the blocks listed in faulty_blocks (default: all)"""
    fb = range(len(blocks)) if faulty_blocks is None else faulty_blocks
    return sum(resblock_padded(x, n, [(dbl(c1), dbl(c2)) for c1, c2 in blk], RESBLOCK_DILS, fault=fault if j in fb else None)
               for j, blk in enumerate(blocks)) / len(blocks)
