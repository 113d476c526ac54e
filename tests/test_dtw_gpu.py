"""GPU: the DTW kernel (ops.dtw over cvx_dtw_f32, csrc/dtw.hip) against the numpy restatement (dtw_restated.py) - cost by torch.equal on
the fp32 bits, steps by integer equality - and the metrics built on it: mel_cepstrum, mel_cepstral_distortion,
CoVoMixModel.evaluate_acoustic and tools/eval_mel.py end to end.  The models here have random weights: no MCD figure printed by these
tests says anything about audio quality."""
import importlib.util
import json
import math
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
import dtw_restated as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
FILL = 0x5A5A5A5A
LENGTHS = [0, 1, 2, 255, 256, 257, 511, 512, 513, 700]          # the issue's lengths
EDGES = (0, 1, 256, 257)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _check(feats, pairs, device_side=False, memo=None):
    from covomix_amd import ops
    cost, steps = ops.dtw([_f32(f).to(DEV) if device_side else _f32(f) for f in feats], pairs)
    want_c, want_s = rs.dtw_many(feats, pairs, memo)
    assert cost.dtype == torch.float32 and steps.dtype == torch.int32 and cost.device.type == steps.device.type == "cpu"
    assert cost.shape == steps.shape == (len(pairs),)
    bad = [(p, float(c), float(wc), int(s), int(ws)) for p, c, wc, s, ws in zip(pairs, cost, want_c, steps, want_s)
           if c.numpy().tobytes() != wc.tobytes() or s != ws]
    assert not bad, bad[:8]
    assert torch.equal(cost.view(torch.int32), torch.from_numpy(want_c).view(torch.int32)) and torch.equal(steps, torch.from_numpy(want_s))
    return cost, steps


def _long_short(pairs, lengths):
    """long and short blocks as neighbours: the costliest pair, the cheapest, the second costliest, ..."""
    order = sorted(pairs, key=lambda p: lengths[p[0]] * lengths[p[1]] + lengths[p[0]] + lengths[p[1]])
    out = []
    while order:
        out.append(order.pop())
        if order:
            out.append(order.pop(0))
    return out


def test_length_edges_in_one_call():
    """every length against 0, 1, 256 and 257 and against its neighbour in the list, D = 13, long and short pairs interleaved; one pair
    4096 x 257 (two bands would need 1025 rows at this width: test_every_width_bucket) and one 4096 x 1"""
    rng = np.random.RandomState(0)
    lens = LENGTHS + [4096]
    feats = [rng.standard_normal((n, 13)).astype(np.float32) for n in lens]
    pairs = [(i, j) for i in range(len(LENGTHS)) for j in range(i, len(LENGTHS))
             if LENGTHS[i] in EDGES or LENGTHS[j] in EDGES or j == i + 1]
    pairs += [(len(LENGTHS), LENGTHS.index(257)), (LENGTHS.index(1), len(LENGTHS))]
    pairs = _long_short(pairs, lens)
    assert 35 <= len(pairs) <= 50
    cost, steps = _check(feats, pairs)
    print("FIGURE (frames, frames, cost, steps) at the length edges:",
          sorted((lens[i], lens[j], round(float(c), 3), int(s)) for (i, j), c, s in zip(pairs, cost, steps))[-5:])


def test_every_width_bucket():
    """D = 1, 13, 16, 17, 32, 33, 79, 80 at 300 x 257 (the widest instance holds one row a thread: 257 rows are two bands there), the
    D = 13 pair embedded in every width with zero columns (bit-identical across D), and pairs whose shorter side needs two bands in
    the instances that hold four rows a thread (1025 and 1100 rows)"""
    from covomix_amd import ops
    rng = np.random.RandomState(1)
    x13, y13 = rng.standard_normal((300, 13)).astype(np.float32), rng.standard_normal((257, 13)).astype(np.float32)
    base = _check([x13, y13], [(0, 1), (1, 0)])
    for d in (1, 13, 16, 17, 32, 33, 79, 80):
        x, y = rng.standard_normal((300, d)).astype(np.float32), rng.standard_normal((257, d)).astype(np.float32)
        _check([x, y], [(0, 1), (1, 0), (1, 1)])
        if d > 13:
            xe, ye = (np.concatenate([v, np.zeros((v.shape[0], d - 13), np.float32)], axis=1) for v in (x13, y13))
            cost, steps = ops.dtw([_f32(xe), _f32(ye)], [(0, 1), (1, 0)])
            assert torch.equal(cost.view(torch.int32), base[0].view(torch.int32)) and torch.equal(steps, base[1]), d
    for d in (13, 20):
        feats = [rng.standard_normal((n, d)).astype(np.float32) for n in (1100, 1025, 3)]
        _check(feats, [(0, 1), (2, 0), (1, 0)])


def test_ties_and_constructed_results():
    from covomix_amd import ops
    rng = np.random.RandomState(2)
    x = rng.standard_normal((300, 13)).astype(np.float32)
    xi = rng.randint(-40, 40, size=(411, 1)).astype(np.float32)
    yi = rng.randint(-40, 40, size=(280, 1)).astype(np.float32)
    small = rng.randint(0, 3, size=(600, 2)).astype(np.float32)          # few distinct values: equal costs on many paths
    feats = [x, np.repeat(x, 2, axis=0), np.full((5, 3), 1.5, np.float32), np.full((9, 3), 1.5, np.float32), xi, yi, small, small[::-1][:500].copy()]
    for group in ([0, 1], [2, 3], [4, 5], [6, 7]):                        # one call per feature size
        f = [feats[i] for i in group]
        cost, steps = _check(f, [(0, 0), (0, 1), (1, 0), (1, 1)])
        if group == [0, 1]:
            assert cost.tolist() == [0.0] * 4 and steps.tolist() == [300, 600, 600, 600]
        if group == [2, 3]:
            assert cost.tolist() == [0.0] * 4 and steps.tolist() == [5, 9, 9, 9]
        if group == [4, 5]:
            assert float(cost[1]) == rs.dtw64(xi, yi)                     # integer 1-D features: exact
    assert [v.tolist() for v in ops.dtw([_f32(x), _f32(x[:0])], [(0, 1), (1, 1), (1, 0)])] == [[0.0, 0.0, 0.0], [0, 0, 0]]


def test_independence():
    """a pair alone, among neighbours and repeated in the table; (a, b) against (b, a); device-side against host-side features; run to run"""
    from covomix_amd import ops
    rng = np.random.RandomState(4)
    feats = [rng.standard_normal((n, 13)).astype(np.float32) for n in (700, 650, 30, 0, 1300)]
    mid = [(0, 2), (2, 4), (1, 1), (3, 4), (4, 1), (3, 3), (2, 2), (0, 4)]
    pairs = [(0, 1)] + mid[:4] + [(0, 1)] + mid[4:] + [(0, 1)]
    memo = {}
    cost, steps = _check(feats, pairs, memo=memo)
    assert cost[0] == cost[5] == cost[-1] and cost[0] > 0 and steps[0] == steps[5] == steps[-1]
    rc, rs_ = _check(feats, [(j, i) for i, j in reversed(pairs)], memo=memo)          # the table turned round, every pair swapped
    assert torch.equal(rc.view(torch.int32), cost.flip(0).view(torch.int32)) and torch.equal(rs_, steps.flip(0))
    for k in (0, 2, 5):                                                                # alone, in a pool of its own
        i, j = pairs[k]
        c1, s1 = ops.dtw([_f32(feats[i]), _f32(feats[j])], [(0, 1)])
        assert c1.view(torch.int32)[0] == cost.view(torch.int32)[k] and s1[0] == steps[k]
    dc, ds = _check(feats, pairs, device_side=True, memo=memo)
    again = ops.dtw([_f32(f) for f in feats], pairs)
    assert torch.equal(again[0].view(torch.int32), cost.view(torch.int32)) and torch.equal(again[1], steps)


def _raw(lib, pool, n_rows, dim, items, pairs, cost, steps, items_dev=None, pairs_dev=None, ld=None):
    from covomix_amd import ops
    it = torch.tensor(items, dtype=torch.int32).reshape(-1, 2)
    pr = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2)
    it_d = (it if items_dev is None else torch.tensor(items_dev, dtype=torch.int32).reshape(-1, 2)).to(DEV)
    pr_d = (pr if pairs_dev is None else torch.tensor(pairs_dev, dtype=torch.int32).reshape(-1, 2)).to(DEV)
    rc = lib.cvx_dtw_f32(pool.data_ptr(), n_rows, pool.shape[1] if ld is None else ld, dim, it.data_ptr(), it_d.data_ptr(), it.shape[0],
                         pr.data_ptr(), pr_d.data_ptr(), pr.shape[0], cost.data_ptr(), steps.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    return rc


def test_overlapping_items_in_a_pool_of_nan():
    """items that overlap, touch and repeat in one pool; every row outside the items and every column [dim, ld) is NaN, and rows behind
    n_rows as well: none of it reaches a result"""
    from covomix_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(5)
    dim, ld, n_rows = 13, 20, 1200
    pool = np.full((n_rows + 300, ld), np.nan, dtype=np.float32)
    items = [(10, 300), (100, 300), (310, 257), (310, 257), (600, 1), (700, 0), (800, 400)]
    for row, n in items:
        pool[row:row + n, :dim] = rng.standard_normal((n, dim)).astype(np.float32)       # later items overwrite the overlap: read below
    feats = [pool[row:row + n, :dim].copy() for row, n in items]
    assert np.isnan(pool[:10]).all() and np.isnan(pool[:, dim:]).all() and np.isnan(pool[n_rows:]).all() and not np.isnan(np.concatenate(feats)).any()
    pairs = [(0, 1), (1, 2), (2, 3), (4, 6), (5, 6), (6, 0), (1, 0), (3, 6)]
    want_c, want_s = rs.dtw_many(feats, pairs)
    cost = torch.full((len(pairs),), FILL, dtype=torch.int32, device=DEV)
    steps = torch.full((len(pairs),), FILL, dtype=torch.int32, device=DEV)
    assert _raw(lib, torch.from_numpy(pool).to(DEV), n_rows, dim, items, pairs, cost.view(torch.float32), steps) == 0
    assert torch.equal(cost.cpu(), torch.from_numpy(want_c).view(torch.int32)) and torch.equal(steps.cpu(), torch.from_numpy(want_s))
    assert float(want_c[2]) == 0.0 and int(want_s[2]) == 257 and int(want_s[4]) == 0


def test_refusals_leave_the_outputs_untouched():
    from covomix_amd import _lib, ops
    lib = _lib.load()
    pool = (torch.arange(5000 * 16, dtype=torch.float32, device=DEV) % 7).reshape(5000, 16)
    good = [(0, 4), (4, 0), (4, 6), (10, 1500)]
    cost = torch.full((4,), FILL, dtype=torch.int32, device=DEV)
    steps = torch.full((4,), FILL, dtype=torch.int32, device=DEV)
    fill = cost.clone()
    for what, items, pairs, n_rows, kw in (("4097 frames", [(0, 4097)], [(0, 0)], 5000, {}),
                                           ("first row + frames past the pool", [(0, 4), (4, 7)], [(0, 1)], 10, {}),
                                           ("negative first row", [(-1, 4)], [(0, 0)], 10, {}),
                                           ("negative frames", [(0, -1)], [(0, 0)], 10, {}),
                                           ("pair index = n_items", good, [(0, 1), (0, 4)], 5000, {}),
                                           ("negative pair index", good, [(0, 1), (-1, 0)], 5000, {}),
                                           ("a bad item no pair names", good + [(4999, 2)], [(0, 1)], 5000, {}),
                                           ("negative n_rows", good[:3], [(0, 1)], -1, {}),
                                           ("dim 0", good, [(0, 2)], 5000, dict(dim=0)),
                                           ("dim past ld", good, [(0, 2)], 5000, dict(dim=17)),
                                           ("ld % 4", good, [(0, 2)], 5000, dict(ld=18))):
        assert _raw(lib, pool, n_rows, kw.get("dim", 13), items, pairs, cost.view(torch.float32), steps, ld=kw.get("ld")) == EINVAL, what
        assert b"dtw" in lib.cvx_last_error_string() and torch.equal(cost, fill) and torch.equal(steps, fill), what
    misaligned = pool.reshape(-1)[1:1 + 100 * 16].reshape(100, 16)
    assert _raw(lib, misaligned, 100, 13, good[:3], [(0, 2)], cost.view(torch.float32), steps) == EINVAL
    assert torch.equal(cost, fill) and torch.equal(steps, fill)
    # no pairs: success, nothing written; then the same tables with pairs: written
    assert _raw(lib, pool, 5000, 13, good, [], cost.view(torch.float32), steps) == 0 and torch.equal(cost, fill) and torch.equal(steps, fill)
    pairs = [(0, 1), (0, 2), (3, 3), (2, 3)]
    feats = [pool[r:r + n, :13].cpu().numpy() for r, n in good]
    want_c, want_s = rs.dtw_many(feats, pairs)
    assert _raw(lib, pool, 5000, 13, good, pairs, cost.view(torch.float32), steps) == 0
    assert torch.equal(cost.cpu(), torch.from_numpy(want_c).view(torch.int32)) and steps.tolist() == want_s.tolist()
    assert steps.tolist()[0] == 0 and steps.tolist()[2] == 1500
    # a device copy that is not the host copy: those blocks read no frame and store (NaN, -1); their neighbours are not touched by that
    for kw, hit in ((dict(pairs_dev=[(0, 1), (0, 4), (3, 3), (-1, 3)]), [1, 3]),
                    (dict(items_dev=[(0, 4), (4, 0), (4998, 6), (10, 4097)]), [1, 2, 3])):
        cost.copy_(fill), steps.copy_(fill)
        assert _raw(lib, pool, 5000, 13, good, pairs, cost.view(torch.float32), steps, **kw) == 0
        c, s = cost.cpu().view(torch.float32), steps.cpu()
        for k in range(4):
            if k in hit:
                assert math.isnan(float(c[k])) and int(s[k]) == -1, (kw, k)
            else:
                assert c[k].numpy().tobytes() == want_c[k].tobytes() and int(s[k]) == int(want_s[k]), (kw, k)
    with pytest.raises(ValueError):
        ops.dtw([torch.zeros(4097, 13)], [(0, 0)])


# ---------------------------------------------------------------- the metrics
def _mels(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, 80, generator=g) * 2.0 - 6.0).clamp(-11.52, 2.0) for n in lengths]


def test_mel_cepstrum_against_fp64_and_alone():
    """within the bound oracle/gemm_f32_oracle.py derives for the fp32 GEMM, (K + 2) 2^-23 (|a| |w|^T) element by element; an item's
    cepstra bit-identical alone and in a batch"""
    from gemm_f32_oracle import U
    from covomix_amd import metrics
    mels = _mels([1, 37, 0, 300, 700, 1500], seed=6)
    got = metrics.mel_cepstrum(mels)
    w = metrics.dct_matrix().double()
    assert [tuple(c.shape) for c in got] == [(m.shape[0], 13) for m in mels] and all(c.is_cuda and c.dtype == torch.float32 for c in got)
    worst = 0.0
    for m, c in zip(mels, got):
        if m.shape[0]:
            err = (c.double().cpu() - m.double() @ w.T).abs()
            bound = (80 + 2) * U * (m.double().abs() @ w.abs().T)
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all())
    print(f"FIGURE mel_cepstrum against fp64: worst |error| / bound = {worst:.4f}")
    for k in (0, 1, 3, 4):
        alone = metrics.mel_cepstrum([mels[k].to(DEV)])[0]
        assert torch.equal(alone, got[k]), k


def test_mel_cepstral_distortion_is_the_restatement_composed_by_hand():
    from covomix_amd import metrics
    pred, ref = _mels([300, 0, 411, 64, 200], seed=7), _mels([257, 50, 380, 0, 200], seed=8)
    ref[4] = pred[4] + 0.25                                      # a constant offset in every bin: only c_0 sees it, which is dropped
    mcd, steps = metrics.mel_cepstral_distortion(pred, ref)
    assert mcd.dtype == torch.float64 and steps.dtype == torch.int32 and mcd.device.type == steps.device.type == "cpu"
    cep = [c.cpu().numpy() for c in metrics.mel_cepstrum(pred + ref)]
    for k in range(5):
        cost, n = rs.dtw(cep[k], cep[5 + k])
        want = rs.mcd(cost, n)
        assert int(steps[k]) == n and (float(mcd[k]) == want or (math.isnan(want) and math.isnan(float(mcd[k])))), k
    assert math.isnan(float(mcd[1])) and math.isnan(float(mcd[3])) and steps.tolist()[1] == steps.tolist()[3] == 0
    assert float(mcd[4]) < 1e-2 and int(steps[4]) >= 200         # rounding noise of the GEMM, against tens of dB between unrelated mels
    print(f"FIGURE MCD of random mels (this project's definition; random data, nothing about audio quality): {[round(float(v), 3) for v in mcd]}")
    # no alignment: the diagonal
    none, n_steps = metrics.mel_cepstral_distortion(pred[4:] + pred[:1], ref[4:] + [pred[0].flip(0).contiguous()], align="none")
    assert n_steps.tolist() == [200, 300]
    d = (torch.from_numpy(cep[0]).double() - torch.from_numpy(cep[0]).flip(0).double()).square().sum(1).sqrt().sum()
    assert abs(float(none[1]) - rs.MCD_CONST * float(d) / 300) <= 1e-5 * float(none[1]) and float(none[0]) < 1e-2
    with pytest.raises(ValueError, match="align='none'"):
        metrics.mel_cepstral_distortion(pred[:1], ref[:1], align="none")


# ---------------------------------------------------------------- the facade
def _acoustic(kind):
    """(model, ids, cond mels, ground-truth mels, y0): utterances of three lengths"""
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel
    from test_model_gpu import _state
    sd = _state(kind, dim=128, dim_emb=64, depth=4, heads=2)
    model = CoVoMixModel.from_state_dict(sd, nfe=4).eval().to(DEV)
    if kind == "vomix":
        g = np.load(os.path.join(GOLDEN, "acoustic_vomix_small.npz"))
        ids, y0 = torch.from_numpy(g["phoneme_ids"]), torch.from_numpy(g["y0"])
        full = syn.synthetic_inputs("vomix", ids.shape[0], ids.shape[1], ids.shape[1], seed=21)["cond"]       # mel in every frame
    else:
        inp = syn.synthetic_inputs("vosingle", 3, 160, 160, seed=22)
        ids, y0, full = inp["phoneme_ids"], inp["y0"], inp["cond"]
    lens = [ids.shape[1], ids.shape[1] * 3 // 4 + 1, 97]
    cut = lambda t: [t[b, :n].contiguous() for b, n in enumerate(lens)]
    gt = _mels(lens, seed=23)                                     # the 'mix mel' of the two-condition model; any target for the other
    return model, cut(ids), cut(full), gt, cut(y0)


@pytest.fixture(scope="module", params=["vomix", "vosingle"])
def acoustic(request):
    return _acoustic(request.param)


@pytest.mark.parametrize("region", [("head", 0.7), ("tail", 0.5)])
def test_evaluate_acoustic_is_sample_then_mse(acoustic, region):
    from covomix_amd import metrics
    model, ids, cond, gt, y0 = acoustic
    res = model.evaluate_acoustic(ids, cond, gt_mels=gt, region=region, cond_scale=0.7, y0=y0, mcd=True)
    assert len(res) == 3 and res[0] == 0.0 and isinstance(res[0], float) and isinstance(res[1], float)
    parts, conds = [], []
    for i_, c in zip(ids, cond):
        k = int(len(i_) * region[1])
        parts.append(slice(0, k) if region[0] == "head" else slice(k, len(i_)))
        c = c.clone()
        c[parts[-1]] = 0
        conds.append(c.to(DEV))
    pred = model.synthesis_sample([i_.to(DEV) for i_ in ids], conds, None, 0.7, y0=y0)
    mse = [F.mse_loss(p[s], g[s].to(DEV)) for p, g, s in zip(pred, gt, parts)]
    want = float(torch.stack([m.double().cpu() for m in mse]).mean())
    print(f"FIGURE evaluate_acoustic {region}: MSE {res[1]:.6f}, MCD without alignment {[round(float(v), 3) for v in res[2]]} dB "
          "(random weights: nothing about audio quality)")
    assert res[1] == want and res[1] > 0
    mcd = metrics.mel_cepstral_distortion([p[s].contiguous() for p, s in zip(pred, parts)], [g[s].contiguous() for g, s in zip(gt, parts)],
                                          align="none")[0]
    assert torch.equal(res[2], mcd) and res[2].dtype == torch.float64 and res[2].shape == (3,)
    two = model.evaluate_acoustic(ids, cond, gt_mels=gt, region=region, y0=y0)
    assert two == (0.0, res[1])
    if cond[0].shape[1] == 80:                                     # gt_mels defaults to the conditioning mels
        dflt = model.evaluate_acoustic(ids, cond, region=region, y0=y0)
        assert dflt[1] == float(torch.stack([F.mse_loss(p[s], c[s].to(DEV)).double().cpu() for p, c, s in zip(pred, cond, parts)]).mean())
    else:
        with pytest.raises(ValueError, match="ground truth"):
            model.evaluate_acoustic(ids, cond, region=region, y0=y0)


def test_evaluate_acoustic_refuses_a_text2semantic_model():
    from covomix_amd.conditional_model import CoVoMixModel
    from test_t2s_filters import load_small
    g, sd = load_small("cosingle_small")
    m = CoVoMixModel(sd, hparams={"text2semantic": True}).eval().to(DEV)
    with pytest.raises(TypeError, match="text2semantic"):
        m.evaluate_acoustic([torch.ones(10, dtype=torch.int64)], [torch.zeros(10, 80)])


# ---------------------------------------------------------------- the tool
def test_eval_mel_end_to_end(tmp_path):
    """three short synthetic wavs against their own .mel.npy (MCD 0 along the diagonal), against the .mel.npy of another signal, and
    against a wav; one file without a partner"""
    from covomix_amd import mel, metrics
    spec = importlib.util.spec_from_file_location("eval_mel", os.path.join(ROOT, "tools", "eval_mel.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pred, ref = tmp_path / "pred", tmp_path / "ref"
    pred.mkdir(), ref.mkdir()
    rng = np.random.RandomState(9)

    def write(path, seconds, f0):
        t = np.arange(int(mel.SR * seconds)) / mel.SR
        x = 0.3 * np.sin(2 * np.pi * f0 * t * (1 + 0.2 * t)) + 0.02 * rng.standard_normal(t.size)
        with wave.open(str(path), "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(mel.SR)
            w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())
    write(pred / "a.wav", 0.9, 220), write(pred / "b.wav", 1.3, 330), write(pred / "c.wav", 0.7, 440), write(pred / "d.wav", 0.5, 500)
    write(ref / "c.wav", 1.0, 392)
    write(tmp_path / "other.wav", 1.1, 300)
    np.save(ref / "a.mel.npy", mel.extract_mel(str(pred / "a.wav")).numpy())
    np.save(ref / "b.mel.npy", mel.extract_mel(str(tmp_path / "other.wav")).numpy())
    out = tmp_path / "out.json"
    assert tool.main(["--pred_dir", str(pred), "--ref_dir", str(ref), "--json", str(out)]) == 0
    res = json.load(open(out))
    assert [r["stem"] for r in res["pairs"]] == ["a", "b", "c"] and res["missing_in_ref_dir"] == ["d"] and res["missing_in_pred_dir"] == []
    to = lambda p: mel.extract_mel(str(p)).t().contiguous()
    want, steps = metrics.mel_cepstral_distortion([to(pred / "a.wav"), to(pred / "b.wav"), to(pred / "c.wav")],
                                                  [to(pred / "a.wav"), to(tmp_path / "other.wav"), to(ref / "c.wav")])
    assert [r["mcd_db"] for r in res["pairs"]] == want.tolist() and [r["steps"] for r in res["pairs"]] == steps.tolist()
    a = res["pairs"][0]
    assert a["mcd_db"] == 0.0 and a["steps"] == a["pred_frames"] == a["ref_frames"] == 45
    assert res["pairs"][1]["mcd_db"] > 0 and res["pairs"][1]["steps"] >= max(res["pairs"][1]["pred_frames"], res["pairs"][1]["ref_frames"])
    assert res["mean_mcd_db"] == sum(want.tolist()) / 3 and res["align"] == "dtw" and res["n_coef"] == 13
    print(f"FIGURE eval_mel on synthetic chirps (nothing about audio quality): {[(r['stem'], round(r['mcd_db'], 3), r['steps']) for r in res['pairs']]}")
