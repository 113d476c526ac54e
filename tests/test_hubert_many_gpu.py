"""GPU: the ragged-batch form of the HuBERT prompt tokeniser (cvx_hubert_extract_features_many and its stepping stones, csrc/hubert.hip;
HubertEncoder.extract_features_many ... tokenize_directory(batch=) in hubert.py) against the fp64 oracle of every item ALONE.

Batch A, items (frames T, remainder r), n = 320 (T - 1) + 400 + r samples, 330 frames in all, a 399-sample (0-frame) item in the middle:
    (1, 0) smallest item; (1, 245) / (1, 250) conv0 output at 128 / 129 rows, the statistics chunk edge; (16, 319) longest slack;
    (17, 1) conv0's 16-frame block edge; (128, 0) / (129, 160) one / two 128-query attention blocks; (37, 7) odd remainder.
Batch B, frames [300, 129, 256, 200, 145] = 1030: past the 1024-row step of tests/hubert_routes.py, items longer than one attention block.

Bounds: over the concatenation the existing FEAT_TOL; per item max(FEAT_TOL, 2 x the distance of the one-utterance extract_features on
the same waveform) - a one-frame item has no averaging over frames, and the one-utterance path is the yardstick there (factor 2 for a
different accumulation route at a different M).  Labels: identical to fp64 wherever the fp64 runner-up margin exceeds 3e-2 (centres near
the features) / 7e-2 (N(0, 1) centres), tests/test_hubert_length_gpu.py's bounds.

Measured on MI355X, relative L2 against fp64, batched / one-utterance call of the same waveform:
    batch A layer 1:  items 1.10e-6 ... 1.62e-6 / 9.7e-7 ... 1.51e-6, all 330 frames 1.58e-6
    batch A layer 12: one-frame items 1.46e-6 ... 1.64e-6 / 1.33e-6 ... 1.50e-6, longer items 5.8e-6 ... 8.1e-6 / 5.0e-6 ... 6.7e-6,
                      all 330 frames 6.84e-6; labels: safe share 1.0 for both centre sets (330 and 18 distinct labels), 0 mismatches
    batch B layer 2:  items 2.00e-6 ... 2.14e-6, all 1030 frames 2.05e-6
    conv0 with statistics per item: 1.07e-7 ... 1.44e-7
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hubert_oracle as ho
from covomix_amd import synthetic

pytestmark = pytest.mark.gpu
FEAT_TOL = {1: 3e-6, 2: 1.2e-5, 12: 3e-5}
ITEMS_A = [(1, 0), (1, 245), (1, 250), (16, 319), (17, 1), (128, 0), (129, 160), (37, 7)]
EMPTY_AT = 4                                             # the 399-sample item sits in front of ITEMS_A[4]
FRAMES_B = [300, 129, 256, 200, 145]


def n_samples(T, r=0):
    return 320 * (T - 1) + 400 + r


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def waveform(n, seed, amp=1.0):
    """tests/test_hubert_length_gpu.py's recipe: two sinusoids, seeded noise and a DC offset."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / 16000.0
    return amp * (0.1 * torch.sin(2 * np.pi * 220 * t) + 0.05 * torch.sin(2 * np.pi * 1710 * t + 0.3) + 0.02 * torch.randn(n, generator=g) + 0.01)


def with_empty(waves):
    return waves[:EMPTY_AT] + [waveform(399, 2000)] + waves[EMPTY_AT:]


@pytest.fixture(scope="module")
def sd():
    return synthetic.hubert_state_dict(seed=0)


@pytest.fixture(scope="module")
def enc(sd):
    from covomix_amd.hubert import HubertEncoder
    return HubertEncoder(sd)


@pytest.fixture(scope="module")
def batch_a(sd, enc):
    """(waveforms of the eight items, their fp64 features {1, 12} each alone): computed once, never modified."""
    waves = [waveform(n_samples(T, r), 1000 + i) for i, (T, r) in enumerate(ITEMS_A)]
    for w, (T, _r) in zip(waves, ITEMS_A):
        assert enc.n_frames(w.numel()) == ho.frames_for(w.numel()) == T
    with torch.no_grad():
        f64 = [ho.get_feats(sd, w.numpy(), layers=(1, 12), dtype=torch.float64) for w in waves]
    return waves, f64


def run_a(enc, waves, layer):
    """Batch A with the empty item inserted, output pre-filled with NaN -> the eight items' features."""
    from covomix_amd import ops
    out = torch.full((sum(T for T, _ in ITEMS_A), 768), float("nan"), device="cuda")
    ops.saturation_reset()
    got = enc.extract_features_many(with_empty(waves), output_layer=layer, out=out)
    assert ops.saturation_query() == 0                                  # the stream's sticky flag is clear after the call
    assert len(got) == len(ITEMS_A) + 1 and got[EMPTY_AT].shape == (0, 768)
    assert bool(torch.isfinite(out).all())                              # fully written
    got = got[:EMPTY_AT] + got[EMPTY_AT + 1:]
    assert [tuple(g.shape) for g in got] == [(T, 768) for T, _ in ITEMS_A]
    return got


@pytest.mark.parametrize("layer", [1, 12])
def test_batch_a_features_vs_fp64(enc, batch_a, layer):
    waves, f64 = batch_a
    got = run_a(enc, waves, layer)
    failures = []
    for i, ((T, r), w, g, ref) in enumerate(zip(ITEMS_A, waves, got, f64)):
        e, e1 = rel(g, ref[layer]), rel(enc.extract_features(w.cuda(), output_layer=layer), ref[layer])
        print(f"hubert many A layer {layer} item {i} (T={T}, r={r}): batched {e:.3e} one-utterance {e1:.3e}")
        if not e < max(FEAT_TOL[layer], 2 * e1):
            failures.append((i, e, e1))
    e = rel(torch.cat(got), torch.cat([ref[layer] for ref in f64]))
    print(f"hubert many A layer {layer} all 330 frames: {e:.3e}")
    assert not failures, failures
    assert e < FEAT_TOL[layer]


def fp64_labels_and_margin(centers, feats64):
    C = torch.from_numpy(np.ascontiguousarray(np.asarray(centers).T)).double()
    dist = feats64.pow(2).sum(1, keepdim=True) - 2 * feats64 @ C + (C ** 2).sum(0, keepdim=True)
    two = dist.topk(2, dim=1, largest=False).values
    return dist.argmin(1).numpy(), (two[:, 1] - two[:, 0]).numpy()


def test_batch_a_labels_of_the_packed_features(enc, batch_a):
    from covomix_amd.hubert import ApplyKmeans
    waves, f64 = batch_a
    f = torch.cat(run_a(enc, waves, 12))
    ref = torch.cat([r[12] for r in f64])
    for tag, centers, bound in (("near", synthetic.hubert_kmeans_centers_near(ref.float().numpy(), seed=0), 3e-2),
                                ("normal", synthetic.hubert_kmeans_centers(seed=0), 7e-2)):
        want, margin = fp64_labels_and_margin(centers, ref)
        got = ApplyKmeans(centers)(f)
        safe = margin > bound
        print(f"hubert many labels {tag}: safe share {safe.mean():.4f}, {len(np.unique(want))} distinct labels, mismatches "
              f"{(got != want).sum()} (on safe frames {(got[safe] != want[safe]).sum()})")
        assert got.shape == want.shape == (330,) and got.dtype == np.int64
        assert safe.mean() >= 0.99
        np.testing.assert_array_equal(got[safe], want[safe])


@pytest.mark.parametrize("keep", [0, 5, 7], ids=["first", "middle", "last"])
def test_an_item_does_not_depend_on_its_neighbours(enc, batch_a, keep):
    """Every OTHER item replaced by another waveform of the same length at 30 x the amplitude: the kept item's layer-12 features are
    bit-identical.  Leaked GroupNorm statistics, halos or attention keys would show here."""
    waves, _ = batch_a
    base = run_a(enc, waves, 12)[keep].clone()
    other = [w if i == keep else waveform(w.numel(), 5000 + i, amp=30.0) for i, w in enumerate(waves)]
    from covomix_amd import ops
    ops.saturation_reset()
    got = enc.extract_features_many(with_empty(other), output_layer=12)
    got = got[:EMPTY_AT] + got[EMPTY_AT + 1:]
    assert bool(torch.isfinite(torch.cat(got)).all())
    assert torch.equal(got[keep], base)
    assert not torch.equal(got[(keep + 1) % len(waves)], run_a(enc, waves, 12)[(keep + 1) % len(waves)])   # the others did change


def test_batch_b_layer_2_vs_fp64(sd, enc):
    waves = [waveform(n_samples(T), 3000 + i) for i, T in enumerate(FRAMES_B)]
    assert [enc.n_frames(w.numel()) for w in waves] == [ho.frames_for(w.numel()) for w in waves] == FRAMES_B
    with torch.no_grad():
        f64 = [ho.get_feats(sd, w.numpy(), layers=(2,), dtype=torch.float64)[2] for w in waves]
    out = torch.full((sum(FRAMES_B), 768), float("nan"), device="cuda")
    got = enc.extract_features_many(waves, output_layer=2, out=out)
    assert bool(torch.isfinite(out).all())
    errs = [rel(g, ref) for g, ref in zip(got, f64)]
    e = rel(out, torch.cat(f64))
    print("hubert many B layer 2 per item: " + " ".join(f"{x:.3e}" for x in errs) + f"; all 1030 frames: {e:.3e}")
    assert max(errs) < FEAT_TOL[2] and e < FEAT_TOL[2]


@pytest.fixture(scope="module")
def short(sd):
    """A 3-frame waveform (1040 samples: 207 conv0 rows) and its fp64 layer-1 features."""
    w = waveform(n_samples(3), 8000)
    with torch.no_grad():
        return w, ho.get_feats(sd, w.numpy(), layers=(1,), dtype=torch.float64)[1]


@pytest.mark.parametrize("lead,tail", [(None, 0), (None, 1), (None, 4), (None, 5), (None, 9), (0, None), (0, 3), (4, 0)])
def test_items_shorter_than_one_conv0_stride_at_the_ends(enc, short, lead, tail):
    """A last item of 0 ... 4 samples starts BEHIND the last conv0 row of the packed buffer (1280 + 4 samples are 255 rows, the item
    starts at row 256), a first item of 0 samples shares its start with its neighbour: both are legal and come back empty, and the
    real item keeps its features (the per-item bound of the batches above)."""
    w, ref = short
    waves = ([torch.zeros(lead)] if lead is not None else []) + [w] + ([torch.zeros(tail)] if tail is not None else [])
    out = torch.full((3, 768), float("nan"), device="cuda")
    got = enc.extract_features_many(waves, output_layer=1, out=out)
    k = 0 if lead is None else 1
    assert [tuple(g.shape) for g in got] == [(3, 768) if i == k else (0, 768) for i in range(len(waves))]
    assert bool(torch.isfinite(out).all())
    e, e1 = rel(got[k], ref), rel(enc.extract_features(w.cuda(), output_layer=1), ref)
    print(f"hubert many, short items at the ends (lead {lead}, tail {tail}): batched {e:.3e} one-utterance {e1:.3e}")
    assert e < max(FEAT_TOL[1], 2 * e1)


def test_empty_and_unsupported_forms(sd, enc):
    from covomix_amd.hubert import HubertEncoder
    assert enc.extract_features_many([]) == []
    got = enc.extract_features_many([torch.zeros(399), torch.zeros(5)], output_layer=1)          # nothing but 0-frame items
    assert [tuple(g.shape) for g in got] == [(0, 768), (0, 768)]
    with pytest.raises(NotImplementedError):
        HubertEncoder(sd, stepped=True).extract_features_many([torch.zeros(800)])


# ---------------------------------------------------------------- the stepping stones alone
def test_conv0_with_statistics_per_item(sd):
    """Conv0 + GroupNorm + GELU over a packed waveform, items whose conv0 output is 127 / 128 / 129 rows (the 128-row statistics
    chunk) and 16 / 17 rows (conv0's 16-frame block), against conv1d + group_norm + gelu of every item alone in float64
    (test_conv0_groupnorm_gelu's bound); the rows of no item are zero."""
    from covomix_amd import ops
    rows = [127, 128, 129, 16, 17]
    lens = [(L - 1) * 5 + 10 + r for L, r in zip(rows, (0, 4, 2, 3, 1))]
    offs, end = [], 0
    for n in lens:
        offs.append(-(-end // 320) * 320)
        end = offs[-1] + n
    waves = [waveform(n, 4000 + i, amp=(1.0, 20.0, 0.05, 3.0, 1.0)[i]) for i, n in enumerate(lens)]
    packed = torch.zeros(end)
    for w, o in zip(waves, offs):
        packed[o:o + w.numel()] = w
    w0 = torch.from_numpy(sd["feature_extractor.conv_layers.0.0.weight"])
    gw, gb = (torch.from_numpy(sd[f"feature_extractor.conv_layers.0.2.{k}"]) for k in ("weight", "bias"))
    starts = [o // 5 for o in offs]
    got = ops.hubert_conv0_gn_gelu_many(packed.cuda(), w0.reshape(512, 10).contiguous().cuda(), gw.cuda(), gb.cuda(), 5, starts, rows)
    assert got.shape == ((end - 10) // 5 + 1, 512)
    mine = torch.zeros(got.shape[0], dtype=torch.bool)
    for w, s0, L in zip(waves, starts, rows):
        y = F.conv1d(w.double().view(1, 1, -1), w0.double(), stride=5)
        y = F.gelu(F.group_norm(y, 512, gw.double(), gb.double(), 1e-5))[0].T
        assert y.shape == (L, 512)
        e = rel(got[s0:s0 + L], y)
        print(f"conv0 per-item statistics, {L} rows at {s0}: {e:.3e}")
        assert e < 2e-6
        mine[s0:s0 + L] = True
    assert (~mine).sum() > 0 and bool((got.cpu()[~mine] == 0).all())


def test_ragged_group_pack_and_unpack():
    """T_b in {1, 63, 64, 65} in one table, HuBERT-Base's 16 groups of 48 with halos of 64: exact copies, zero halos (the output
    starts as NaN: halo rows are written), nothing outside the table touched; the unpack adds the residual on compact rows."""
    from covomix_amd import ops
    from covomix_amd.hubert import item_table
    G, cg, k = 16, 48, 128
    D = G * cg
    t = item_table([n_samples(T) for T in (1, 63, 64, 65)])
    assert t.frames.tolist() == [1, 63, 64, 65] and (t.M, t.Mh) == (193, 193 + 4 * k)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(t.M, D, generator=g).cuda()
    buf = torch.full((G * t.Mh * cg + 1000,), float("nan"), device="cuda")
    out = ops.hubert_group_pack_many(x, G, t.pack_src, out=buf[:G * t.Mh * cg].view(G, t.Mh, cg))
    want = torch.zeros(G, t.Mh, cg, dtype=torch.float64)
    xd = x.double().cpu()
    for b, T in enumerate(t.frames.tolist()):
        lo = int(t.cuh[b]) + k // 2
        want[:, lo:lo + T] = xd[int(t.cu[b]):int(t.cu[b]) + T].view(T, G, cg).permute(1, 0, 2)
    assert torch.equal(out.double().cpu(), want)
    halo = torch.from_numpy(t.pack_src < 0)
    assert int(halo.sum()) == 4 * k and bool((out.cpu()[:, halo] == 0).all())
    assert bool(torch.isnan(buf[G * t.Mh * cg:]).all())
    # the im2col window of frame tt of item b = its own rows between zeros: the same as the one-utterance pack of that item
    for b, T in enumerate(t.frames.tolist()):
        alone = ops.hubert_group_pack(x[int(t.cu[b]):int(t.cu[b]) + T].contiguous(), G, k // 2)
        assert torch.equal(out[:, int(t.cuh[b]):int(t.cuh[b]) + T + k], alone)
    conv = torch.randn(t.Mh - k, D, generator=g).cuda()
    xbuf = torch.full((t.M + 5, D), float("nan"), device="cuda")
    got = ops.hubert_group_unpack_add(x, conv, t.unpack, out=xbuf[:t.M])
    want = (xd + conv.double().cpu()[torch.from_numpy(t.unpack.astype(np.int64))]).float()
    assert torch.equal(got.cpu(), want) and bool(torch.isnan(xbuf[t.M:]).all())


def test_row_gather():
    from covomix_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(50, 512, generator=g).cuda()
    row_map = [49, 0, 0, -1, 17, 48, 3] + list(range(20, 45))
    buf = torch.full((len(row_map) + 3, 512), float("nan"), device="cuda")
    got = ops.row_gather(x, row_map, out=buf[:len(row_map)])
    want = torch.stack([x.double().cpu()[r] if r >= 0 else torch.zeros(512, dtype=torch.float64) for r in row_map])
    assert torch.equal(got.double().cpu(), want) and bool(torch.isnan(buf[len(row_map):]).all())


# ---------------------------------------------------------------- end to end, in the reference's file layouts
@pytest.fixture(scope="module")
def files(sd, tmp_path_factory):
    import joblib
    import types
    from scipy.io.wavfile import write
    d = tmp_path_factory.mktemp("hubert_many")
    ckpt, kmp = str(d / "hubert.pt"), str(d / "km.bin")
    torch.save({"cfg": {"model": {"_name": "hubert", "encoder_layers": 12, "encoder_attention_heads": 12, "conv_pos": 128,
                                  "conv_pos_groups": 16, "extractor_mode": "default", "layer_norm_first": False,
                                  "conv_feature_layers": "[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2"},
                        "task": {"_name": "hubert_pretraining", "sample_rate": 16000, "normalize": False}},
                "model": {k: torch.from_numpy(v) for k, v in sd.items()}}, ckpt)
    centers = synthetic.hubert_kmeans_centers(seed=0)
    joblib.dump(types.SimpleNamespace(cluster_centers_=centers), kmp)
    os.makedirs(d / "wavs")
    paths, safe = [], {}
    for i, (T, r, channels) in enumerate([(21, 5, 1), (40, 0, 2), (9, 300, 1), (33, 17, 1)]):
        pcm = np.stack([np.clip(np.round(waveform(n_samples(T, r), 6000 + 10 * i + c).numpy() * 32768.0), -32768, 32767).astype(np.int16)
                        for c in range(channels)], 1)
        path = str(d / "wavs" / f"utt{i}.wav")
        write(path, 16000, pcm[:, 0] if channels == 1 else pcm)
        with torch.no_grad():
            f64 = ho.get_feats(sd, pcm[:, 0].astype(np.float32) / 32768.0, layer=12, dtype=torch.float64)
        safe[f"utt{i}"] = fp64_labels_and_margin(centers, f64)[1] > 7e-2
        paths.append(path)
    return dict(dir=str(d / "wavs"), out=d, ckpt=ckpt, km=kmp, paths=paths, safe=safe)


def same_on_safe_frames(a, b, safe):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    assert a.shape == b.shape == safe.shape
    np.testing.assert_array_equal(a[safe], b[safe])
    assert (a != b).sum() <= (~safe).sum()


def test_wav2code_many_equals_wav2code_file_by_file(files):
    from covomix_amd.hubert import HubertTokenizer
    tok = HubertTokenizer(hubert_path=files["ckpt"], hubert_layer=12, km_path=files["km"])
    many = tok.wav2code_many(files["paths"], channel_id=1)
    assert len(many) == 4 and all(isinstance(c, str) for c in many)
    for path, code in zip(files["paths"], many):
        name = os.path.basename(path)[:-4]
        same_on_safe_frames(code.split(" "), tok.wav2code(path, 1).split(" "), files["safe"][name])
    # a chunked file contributes its chunks as separate items, concatenated as get_feats does
    reader = tok.feature_extractor
    reader.max_chunk = 4000
    wav = waveform(9000, 77).numpy()
    a, b = reader.get_feats_many([wav, wav[:3000]]), [reader.get_feats(wav), reader.get_feats(wav[:3000])]
    assert [tuple(x.shape) for x in a] == [tuple(x.shape) for x in b] == [(2 * ho.frames_for(4000) + ho.frames_for(1000), 768), (ho.frames_for(3000), 768)]
    assert rel(a[0], b[0]) < 3e-5 and rel(a[1], b[1]) < 3e-5
    small = reader.get_feats_many([wav, wav[:3000]], max_batch_samples=4200)          # the budget cuts the list: the same features
    assert all(torch.equal(x, y) for x, y in zip(small[1:], reader.get_feats_many([wav[:3000]])))
    # normalize=True checkpoints: the layer norm runs over every whole file, before it is cut into chunks (the DC offset and the scale
    # of `loud` would otherwise reach the features)
    reader.normalize = True
    loud = 7.0 * wav[:5000] + 0.3
    a, b = reader.get_feats_many([wav, loud]), [reader.get_feats(wav), reader.get_feats(loud)]
    assert [tuple(x.shape) for x in a] == [tuple(x.shape) for x in b]
    assert rel(a[0], b[0]) < 3e-5 and rel(a[1], b[1]) < 3e-5


def test_tokenize_directory_in_batches_writes_the_same_files(files):
    from covomix_amd.hubert import tokenize_directory
    one, three = str(files["out"] / "codes1"), str(files["out"] / "codes3")
    assert tokenize_directory(files["dir"], one, files["ckpt"], files["km"]) == 4
    assert tokenize_directory(files["dir"], three, files["ckpt"], files["km"], batch=3) == 4
    assert sorted(os.listdir(one)) == sorted(os.listdir(three)) == [f"utt{i}.hubert_code.npy" for i in range(4)]
    for name, safe in files["safe"].items():
        a, b = np.load(os.path.join(one, name + ".hubert_code.npy")), np.load(os.path.join(three, name + ".hubert_code.npy"))
        assert a.dtype.kind == b.dtype.kind == "U"
        same_on_safe_frames(b, a, safe)
