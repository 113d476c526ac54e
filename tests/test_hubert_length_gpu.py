"""GPU: the HuBERT prompt tokeniser (csrc/hubert.hip, hubert.py, the plain pre-split GEMM route of csrc/gemm_f16x3.hip) through the C
ABI against the fp64 oracle at 1024, 1025, 2048 and 2049 frames - the frame counts either side of the two thresholds at which the
encoder's GEMMs change launch form.  tests/test_hubert_gpu.py stops at 149 frames; a 10-s prompt is 499 frames, a full
HubertFeatureReader chunk 4999.

Route table (M = T frames; tests/test_hubert_length.py holds it against the library's host arithmetic).  The plain pre-split branch
of gemm_f16x3_impl works in 128 x 128 tiles with tile rows padded to a multiple of 8 (grid_m), splits K 4-fold when the caller
passes a workspace (hubert.hip's lin() and ops.gemm do for M <= 2048), the padded grid has at most 128 tiles and a slice keeps 512
columns, and takes the 4-stage DMA ring when grid.x * ksplit <= 256, else the 2-stage ring at two blocks per CU:

    T            grid_m   4-stage ring          2-stage ring     split-K
    <= 1024      8        all                   none             fc2 x4, pos x4
    1025 .. 2048 16       proj, pos, out        qkv, fc1, fc2    fc2 x4 (on the 2-stage ring), pos x4
    >= 2049      24 ..    proj, pos, out, fc2   qkv, fc1         none (no workspace)

(proj 768 x 512, sixteen pos-conv groups 48 x 6144, qkv 2304 x 768, out 768 x 768, fc1 3072 x 768, fc2 768 x 3072.)  The attention
(cvx_attention_f32, split output) runs 8, 9, 16 and 17 query tiles of 128 per head at these lengths.

What each case is there to launch:
  test_features_vs_fp64[1024]   the last length of the short-audio forms: everything on the 4-stage ring, fc2 and pos split 4-fold
  test_features_vs_fp64[1025]   gemm_f16x3_dma_kernel<2,3> with bias (qkv), with bias + GELU + split output, no fp32 store (fc1), and
                                with k_per (fc2: the 2-stage ring under split-K + splitk_reduce_kernel with bias and residual)
  test_features_vs_fp64[2048]   the same forms on full tiles, the last length with a workspace
  test_features_vs_fp64[2049]   no workspace: fc2 back on <4,3> unsplit over 144 blocks, pos unsplit, qkv / fc1 on <2,3> at 432 / 576 blocks
  test_labels_at_2049_frames    k-means labels of those layer-12 features
  test_stepped_path_equals_the_c_entry_point   hubert.py's and hubert.hip's own M <= 2048 workspace rules, bit for bit
  test_fp32_mode_at_1025_frames cvx_gemm_bias_act_f32 at 1025 rows
  test_encoder_gemm_crossing_shapes / test_pos_conv_operand_crossing / test_single_term_past_256_blocks   the GEMM forms alone

Measured, relative L2 against the fp64 oracle: "kernel" = the default f16x3 path through cvx_hubert_extract_features on MI355X,
"fp32" = the oracle restated in fp32 on the CPU (torch CPU kernels, 16 threads), same waveform:

    T      what       kernel     fp32       kernel / fp32
    1024   layer 1    1.64e-6    7.76e-7    2.1
    1025   conv       1.34e-6    5.14e-7    2.6
    1025   layer 1    1.67e-6    7.80e-7    2.1
    1025   layer 12   5.66e-6    2.79e-6    2.0
    2048   layer 2    2.03e-6    9.28e-7    2.2
    2049   conv       1.39e-6    5.13e-7    2.7
    2049   layer 2    2.15e-6    9.21e-7    2.3
    2049   layer 12   5.68e-6    2.53e-6    2.3
    1025   layer 2, precision="fp32"   3.30e-6   9.55e-7

Every figure is inside its bound and none moves at a threshold (1024 -> 1025, 2048 -> 2049), but the kernel path sits 2.0 to 2.7 times
the fp32 restatement's distance, above the factor of two at which the figures were to be traced.  Traced at T = 1025, every stage on
exact (fp64-derived) inputs: conv layer 0 + GroupNorm + GELU 1.0e-7; each conv-layer GEMM 5.0e-7 on the f16x3 kernel (K = 1536, one
fp32 accumulator through 96 steps of three MFMAs), 4.2e-7 at K = 1024, 3.1e-7 where K splits in two, 8.0e-7 on the library's fp32
MFMA kernel, 1.9e-7 on the CPU's blocked fp32 convolution; the six layers compound to 5.1e-7 -> 1.34e-6.  LayerNorm 6.7e-8 (CPU fp32
7.1e-8), proj 2.6e-7 (2.4e-7), attention 8.8e-7 (4.9e-7).  The distance is the GEMMs' sequential fp32 accumulation over K / 16 steps,
the same at every length (the kernel-level cases below: 5.1e-7 unsplit at K = 3072, 2.6e-7 in four slices); no kernel form reached
past 1024 or 2048 frames adds to it.

Labels at T = 2049, layer 12 (500 centres): centres near the fp64 features: safe share 0.9971, 500 distinct fp64 labels, 0 mismatches
(0 on safe frames); N(0, 1) centres: safe share 0.9985, 25 distinct labels, 0 mismatches.  The fp32 restatement: 0 mismatches for both.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hubert_oracle as ho
from covomix_amd import synthetic
from hubert_routes import LENGTHS, n_samples, route

pytestmark = pytest.mark.gpu
FEAT_TOL = {1: 3e-6, 2: 1.2e-5, 6: 1.2e-5, 12: 3e-5}     # tests/test_hubert_gpu.py's, layer 2 held to layer 6's (error grows with depth)
CONV_TOL = 2e-6
ORACLE_LAYERS = {1024: (1,), 1025: (1, 2, 12), 2048: (2,), 2049: (2, 12)}
CHECKED = {1024: (1,), 1025: (1, 12), 2048: (2,), 2049: (2, 12)}
CONV_CHECKED = (1025, 2049)


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def waveform(T):
    """test_other_lengths_vs_fp64_oracle's recipe (two sinusoids + seeded noise) plus a DC offset, exactly T frames long."""
    n = n_samples(T)
    g = torch.Generator().manual_seed(n)
    t = torch.arange(n) / 16000.0
    return 0.1 * torch.sin(2 * np.pi * 220 * t) + 0.05 * torch.sin(2 * np.pi * 1710 * t + 0.3) + 0.02 * torch.randn(n, generator=g) + 0.01


@pytest.fixture(scope="module")
def sd():
    return synthetic.hubert_state_dict(seed=0)


@pytest.fixture(scope="module")
def enc(sd):
    from covomix_amd.hubert import HubertEncoder
    return HubertEncoder(sd)


@pytest.fixture(scope="module")
def oracle(sd):
    """T -> (waveform, fp64 taps, fp32 taps): one oracle pass per waveform and precision, shared by every test, never modified."""
    cache = {}

    def get(T):
        if T not in cache:
            wav = waveform(T)
            with torch.no_grad():
                f64 = ho.get_feats(sd, wav.numpy(), layers=ORACLE_LAYERS[T], conv=True, dtype=torch.float64)
                f32 = ho.get_feats(sd, wav.numpy(), layers=ORACLE_LAYERS[T], conv=True, dtype=torch.float32)
            cache[T] = (wav, f64, f32)
        return cache[T]
    return get


@pytest.mark.parametrize("T", LENGTHS)
def test_features_vs_fp64(enc, oracle, T):
    """(a) default f16x3 path, one-call C entry point, against the fp64 oracle; the fp32 restatement's own distance printed next to
    it (more than twice that distance would be a finding, not headroom)."""
    wav, f64, f32 = oracle(T)
    n = wav.numel()
    assert ho.frames_for(n) == enc.n_frames(n) == T
    assert not enc.stepped
    dev = wav.cuda()
    for layer in CHECKED[T]:
        f = enc.extract_features(dev, output_layer=layer)
        assert f.shape == (T, 768) == f64[layer].shape
        e, e32 = rel(f, f64[layer]), rel(f32[layer], f64[layer])
        print(f"hubert T={T} layer {layer}: kernel {e:.3e} fp32-restated {e32:.3e} ratio {e / e32:.2f}")
        assert e < FEAT_TOL[layer], (T, layer, e)
    if T in CONV_CHECKED:
        conv = enc.conv_features(dev)
        assert conv.shape == (T, 512) == f64["conv"].shape
        e, e32 = rel(conv, f64["conv"]), rel(f32["conv"], f64["conv"])
        print(f"hubert T={T} conv: kernel {e:.3e} fp32-restated {e32:.3e} ratio {e / e32:.2f}")
        assert e < CONV_TOL, (T, e)


def fp64_labels_and_margin(centers, feats64):
    """ApplyKmeans in fp64 + the runner-up margin of every frame."""
    C = torch.from_numpy(np.ascontiguousarray(np.asarray(centers).T)).double()
    dist = feats64.pow(2).sum(1, keepdim=True) - 2 * feats64 @ C + (C ** 2).sum(0, keepdim=True)
    two = dist.topk(2, dim=1, largest=False).values
    return dist.argmin(1).numpy(), (two[:, 1] - two[:, 0]).numpy()


def test_labels_at_2049_frames(enc, oracle):
    """(b) labels of the layer-12 features at 2049 frames: identical to the fp64 labels wherever the fp64 runner-up margin exceeds
    the distance error a 3e-5 feature error implies (2 |dx| |c_a - c_b|: 2 * 3e-5 * 28 * 14 < 3e-2 for centres near the features,
    2 * 3e-5 * 28 * 39 < 7e-2 for N(0, 1) centres - tests/test_hubert_gpu.py's bounds)."""
    from covomix_amd.hubert import ApplyKmeans
    T = 2049
    wav, f64, f32 = oracle(T)
    f = enc.extract_features(wav.cuda(), output_layer=12)
    for tag, centers, bound in (("near", synthetic.hubert_kmeans_centers_near(f64[12].float().numpy(), seed=0), 3e-2),
                                ("normal", synthetic.hubert_kmeans_centers(seed=0), 7e-2)):
        want, margin = fp64_labels_and_margin(centers, f64[12])
        got = ApplyKmeans(centers)(f)
        safe = margin > bound
        restated = ho.apply_kmeans(centers, f32[12])
        print(f"hubert labels T={T} {tag}: safe share {safe.mean():.4f}, {len(np.unique(want))} distinct labels, kernel mismatches "
              f"{(got != want).sum()} (on safe frames {(got[safe] != want[safe]).sum()}), fp32-restated mismatches {(restated != want).sum()}")
        assert got.shape == want.shape == (T,) and got.dtype == np.int64
        assert safe.mean() >= 0.99
        np.testing.assert_array_equal(got[safe], want[safe])
        assert (got != want).sum() <= (~safe).sum()


@pytest.mark.parametrize("T", LENGTHS)
def test_stepped_path_equals_the_c_entry_point(sd, enc, T):
    """(c) hubert.py (stepped from Python, workspace from ops.gemm) and hubert.hip (one C call, workspace from plan_hubert) each
    apply the M <= 2048 rule themselves: the same kernels with the same arguments, bit-identical features."""
    from covomix_amd.hubert import HubertEncoder
    stepped = HubertEncoder(sd, stepped=True)
    assert stepped.stepped and not enc.stepped
    wav = waveform(T).cuda()
    a, b = enc.extract_features(wav, 2), stepped.extract_features(wav, 2)
    assert a.shape == b.shape == (T, 768) and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)


def test_fp32_mode_at_1025_frames(sd, oracle):
    """(d) precision="fp32" (cvx_gemm_bias_act_f32 throughout) at 1025 frames, layer 2."""
    from covomix_amd.hubert import HubertEncoder
    wav, f64, f32 = oracle(1025)
    f = HubertEncoder(sd, precision="fp32").extract_features(wav.cuda(), output_layer=2)
    e = rel(f, f64[2])
    print(f"hubert fp32 mode T=1025 layer 2: kernel {e:.3e} fp32-restated {rel(f32[2], f64[2]):.3e}")
    assert e < 5e-5


# ---------------------------------------------------------------- (e) the encoder's GEMMs alone, at the crossing shapes
def dev():
    return torch.device("cuda:0")


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev())


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev())


@pytest.mark.parametrize("M,N,K,residual,act,split_only,form", [
    (1025, 768, 3072, True, 0, False, (2, 4)),           # fc2: the 2-stage ring under split-K, reduction with bias + residual
    (2048, 768, 3072, True, 0, False, (2, 4)),           # the same forms on full tiles
    (2049, 768, 3072, True, 0, False, (4, 1)),           # no workspace: 4-stage, unsplit, 144 blocks
    (1025, 2304, 768, False, 0, False, (2, 1)),          # qkv: 2-stage with bias
    (1025, 3072, 768, False, 1, True, (2, 1)),           # fc1: 2-stage, bias + GELU, split output only
])
def test_encoder_gemm_crossing_shapes(M, N, K, residual, act, split_only, form):
    """ops.gemm on the plain pre-split route against fp64 and against the on-the-fly split kernel (the bounds of
    test_gemm_f16x3_presplit_dma_and_split_output), outputs pre-filled with NaN."""
    from covomix_amd import ops
    assert route(M, N, K) == form
    a, w = randn(M, K, seed=M + 1) * 2.0, randn(N, K, seed=M + 2) / math.sqrt(K)
    b = randn(N, seed=M + 3)
    r = randn(M, N, seed=M + 4) if residual else None
    ws, asp = ops.split_f16(w), ops.split_act_f16(a)
    ref = a.double() @ w.double().T + b.double()
    if act:
        ref = F.gelu(ref)
    if residual:
        ref = ref + r.double()
    o1 = nan(M, N)
    ops.gemm(a, w, o1, bias=b, act=act, residual=r, w_split=ws)                         # A split on the fly
    if split_only:
        o2 = torch.full((M, N), 7.0, device=dev())
        oh, ol = nan(M, N, dtype=torch.float16), nan(M, N, dtype=torch.float16)
        ops.gemm(a, w, o2, bias=b, act=act, residual=r, w_split=ws, a_split=asp, out_split=(oh, ol), write_f32=False)
        assert bool((o2 == 7.0).all())                                                  # the fp32 buffer is untouched
        got = oh.float() + ol.float()
    else:
        got = nan(M, N)
        ops.gemm(a, w, got, bias=b, act=act, residual=r, w_split=ws, a_split=asp)
    e, e1 = rel(got, ref), rel(got, o1)
    print(f"pre-split gemm {(M, N, K)} {form}: vs fp64 {e:.3e}, vs on-the-fly {e1:.3e}")
    assert e < 3e-6 and e1 < 1e-6


@pytest.mark.parametrize("T,form", [(1025, (4, 4)), (2049, (4, 1))])
def test_pos_conv_operand_crossing(T, form):
    """The positional convolution's GEMM as the encoder issues it: M = T, N = 48, K = 6144, A = overlapping rows (row stride 48) of
    hubert_group_pack's output, C / bias / residual 48-column slices of [T, 768] tensors, GELU.  The first, a middle and the last
    group (whose last row ends at the end of the packed buffer); columns outside the slice stay untouched."""
    from covomix_amd import ops
    G, cg, k = 16, 48, 128
    assert route(T, cg, k * cg) == form
    h = randn(T, G * cg, seed=T)
    bias = randn(G * cg, seed=T + 1)
    packed = ops.hubert_group_pack(h, G, k // 2)
    p16 = ops.split_act_f16(packed.view(-1, cg))
    x, x1 = nan(T, G * cg), nan(T, G * cg)
    groups = (0, 7, 15)
    for g in groups:
        w = randn(cg, k * cg, seed=T + 10 + g) / math.sqrt(k * cg)
        ws = ops.split_f16(w)
        a = packed[g].as_strided((T, k * cg), (cg, 1), packed[g].storage_offset())
        a16 = tuple(t.as_strided((T, k * cg), (cg, 1), g * (T + k) * cg) for t in p16)
        sl = slice(g * cg, (g + 1) * cg)
        ops.gemm(a, w, x[:, sl], bias=bias[sl], act=ops.ACT_GELU, residual=h[:, sl], w_split=ws, a_split=a16)
        ops.gemm(a, w, x1[:, sl], bias=bias[sl], act=ops.ACT_GELU, residual=h[:, sl], w_split=ws)
        ref = h[:, sl].double() + F.gelu(a.double() @ w.double().T + bias[sl].double())
        e, e1 = rel(x[:, sl], ref), rel(x[:, sl], x1[:, sl])
        print(f"pos-conv gemm T={T} group {g} {form}: vs fp64 {e:.3e}, vs on-the-fly {e1:.3e}")
        assert e < 3e-6 and e1 < 1e-6
    rest = torch.ones(G * cg, dtype=torch.bool, device=dev())
    for g in groups:
        rest[g * cg:(g + 1) * cg] = False
    assert bool(torch.isnan(x[:, rest]).all()) and bool(torch.isnan(x1[:, rest]).all())


def test_single_term_past_256_blocks():
    """W_lo == NULL at (4200, 1024, 1024): 40 padded tile rows x 8 = 320 blocks, the first shape that launches
    gemm_f16x3_dma_kernel<2,1> (test_gemm_f16_single_term's largest is 256 blocks); that test's bounds."""
    from covomix_amd import ops
    M, N, K = 4200, 1024, 1024
    assert route(M, N, K) == (2, 1) and route(4096, N, K) == (4, 1)
    a, w = randn(M, K, seed=200) * 2.0, randn(N, K, seed=201) / math.sqrt(K)
    b, r = randn(N, seed=202), randn(M, N, seed=203)
    wh, wl, inv = ops.split_f16(w, with_lo=False)
    assert wl is None
    ah = torch.empty(M, K, dtype=torch.float16, device=dev())
    ops.split_act_f16(a, ah, None)
    out, oh = nan(M, N), nan(M, N, dtype=torch.float16)
    ops.gemm(a, w, out, bias=b, act=1, residual=r, w_split=(wh, None, inv), a_split=(ah, None), out_split=(oh, None))
    rounded = F.gelu(ah.double() @ (wh.double() * inv).T + b.double()) + r.double()
    exact = F.gelu(a.double() @ w.double().T + b.double()) + r.double()
    e, ex = rel(out, rounded), rel(out, exact)
    print(f"f16 single-term gemm {(M, N, K)}: vs rounded operands {e:.3e}, vs fp64 {ex:.3e}")
    assert e < 3e-6 and ex < 1e-3
    assert torch.equal(oh, out.half())
