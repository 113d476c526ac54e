"""The flow-matching loss on the CPU: the restatement against its formulas in fp64, the mask draws against hand-made cases, the route
of an evaluation with a time per sequence against route(), every refusal of the host layer and the facade, the header / binding, the
new kernels' code objects (no private segment, LDS inside the budget) and the tool's parser and pairing."""
import os
import re

import numpy as np
import pytest
import torch

import flow_loss_restated as rs
from conftest import ROOT

U = 2.0 ** -24          # unit roundoff of fp32
EPS = 2.0 ** -23


# ---------------------------------------------------------------- the restated inputs
@pytest.mark.parametrize("sigma", [0.0, 1e-4])
def test_restated_inputs_match_the_formulas(sigma):
    g = np.random.default_rng(5)
    M, D, C = 97, 80, 160
    x1, x0 = (g.standard_normal((M, D)) * 3).astype(np.float32), g.standard_normal((M, D)).astype(np.float32)
    cond = g.standard_normal((M, C)).astype(np.float32)
    mask = g.random(M) < 0.4
    t = np.concatenate([np.zeros(10), np.ones(10), g.random(M - 20)]).astype(np.float32)
    w, flow, cond_in = rs.cfm_inputs(x1, x0, cond, mask, t, sigma)
    w64, flow64, cond64 = rs.cfm_inputs64(x1, x0, cond, mask, t, sigma)
    assert w.dtype == flow.dtype == cond_in.dtype == np.float32
    # three roundings (eps = 2^-23 each) of the operands' magnitude: c = 1 - (1 - sigma) t carries two, the products and the sum one each
    bound = 3 * EPS * (np.abs(x0.astype(np.float64)) + np.abs(x1.astype(np.float64)))
    assert (np.abs(w - w64) <= bound).all() and (np.abs(flow - flow64) <= bound).all()
    assert (cond_in == cond64).all() and (cond_in[mask] == 0).all() and (cond_in[~mask] == cond[~mask]).all()
    # t = 0: w is x0 exactly at sigma = 0; t = 1: w is x1 exactly (c = 0 at sigma = 0)
    if sigma == 0.0:
        assert (w[:10] == x0[:10]).all() and (w[10:20] == x1[10:20]).all()
        assert (flow == (x1 - x0).astype(np.float32)).all()


def test_masked_loss64_is_the_reference_reduction():
    g = torch.Generator().manual_seed(3)
    pred, flow = torch.randn(9, 80, generator=g), torch.randn(9, 80, generator=g)
    mask = torch.tensor([0, 1, 1, 0, 0, 1, 0, 0, 0], dtype=torch.bool)
    loss, err = rs.masked_loss64(pred, flow, mask)
    ref = torch.nn.functional.mse_loss(pred.double(), flow.double(), reduction="none").mean(-1)
    assert torch.equal(err, ref) and abs(loss - float(ref[mask].sum() / 3)) < 1e-15
    assert rs.masked_loss64(pred, flow, torch.zeros(9, dtype=torch.bool))[0] == 0.0


# ---------------------------------------------------------------- the draws
def test_span_mask_truncates_and_stays_inside():
    from covomix_amd.flow_loss import span_mask
    m = span_mask(10, 0.75, 0.5)                 # int(7.5) = 7 frames from int(3 * 0.5) = 1
    assert m.tolist() == [False] + [True] * 7 + [False] * 2
    assert span_mask(10, 1.0, 0.9).all()         # the whole sequence: start int(0 * u) = 0
    assert span_mask(10, 0.75, 0.999).tolist() == [False] * 2 + [True] * 7 + [False]    # int(2.997) = 2: ends at 9
    assert span_mask(10, 0.7, 0.0).tolist() == [True] * 7 + [False] * 3                 # fp32(0.7) * 10 = 7.0000000
    assert not span_mask(1, 0.7, 0.3).any()      # int(0.7) = 0 frames: an empty mask is a valid draw
    assert span_mask(3, 0.99, 0.999).tolist() == [True, True, False]                   # int(2.97) = 2 frames from int(1 * 0.999) = 0
    for T in (1, 2, 7, 64, 1001):
        for f in (0.7, 0.85, 0.999, 1.0):
            for u in (0.0, 0.5, 0.99999):
                m = span_mask(T, f, u)
                idx = m.nonzero().flatten()
                assert int(m.sum()) == int((torch.tensor(f, dtype=torch.float32) * T).long())
                assert idx.numel() == 0 or (int(idx[-1]) - int(idx[0]) + 1 == idx.numel() and int(idx[-1]) < T)


def test_draws_are_seeded_and_ordered():
    from covomix_amd import flow_loss as fl
    a, b = fl.draw([5, 9, 200], 80, 7), fl.draw([5, 9, 200], 80, 7)
    assert a["times"] == b["times"] and all(torch.equal(x, y) for x, y in zip(a["x0"] + a["masks"], b["x0"] + b["masks"]))
    assert all(0.0 <= t < 1.0 for t in a["times"]) and [x.shape for x in a["x0"]] == [(5, 80), (9, 80), (200, 80)]
    assert fl.draw([5, 9, 200], 80, 8)["times"] != a["times"]
    # a kind the caller passes is skipped: the masks alone are the generator's first draws
    g = torch.Generator().manual_seed(7)
    assert torch.equal(fl.draw([50], 80, 7, need_times=False, need_x0=False)["masks"][0], fl.draw_mask(50, g))
    # both kinds of mask occur, the Bernoulli one near p = 0.3, the span between 70 % and 100 %
    kinds = set()
    for seed in range(40):
        m = fl.draw([400], 80, seed, need_times=False, need_x0=False)["masks"][0]
        idx = m.nonzero().flatten()
        span = idx.numel() and int(idx[-1]) - int(idx[0]) + 1 == idx.numel()
        kinds.add(bool(span))
        frac = float(m.float().mean())
        assert (0.7 - 1 / 400 <= frac <= 1.0) if span else (0.15 < frac < 0.45)
    assert kinds == {True, False}


def test_cut_launches():
    from covomix_amd.flow_loss import cut_launches
    assert cut_launches([5, 5, 5], 10, 4096) == [range(0, 2), range(2, 3)]
    assert cut_launches([50, 5, 5], 10, 4096) == [range(0, 1), range(1, 3)]             # a long utterance runs alone
    assert cut_launches([1] * 5, 100, 2) == [range(0, 2), range(2, 4), range(4, 5)]
    with pytest.raises(ValueError):
        cut_launches([1], 0, 4096)


# ---------------------------------------------------------------- the route
@pytest.mark.parametrize("precision", ["f16x3", "fp32", "f16"])
def test_route_seq_times_is_route_with_three_fields_off(precision, monkeypatch):
    import dataclasses
    from covomix_amd.acoustic import route, route_seq_times
    for M in (1, 64, 65, 127, 128, 2047, 2048, 2049, 8191, 8192, 8193, 20000):
        for ragged in (None, M):
            r, rs_ = route(M, 512, precision, ragged), route_seq_times(M, 512, precision, ragged)
            assert rs_ == dataclasses.replace(r, fuse_norm=False, deferred=False, graph=False)
            assert not (rs_.fuse_norm or rs_.deferred or rs_.graph)
    assert route(8192, 512, "f16x3", 8192).deferred and route(1024, 512, "f16x3").fuse_norm and route(1024, 512, "f16x3").graph
    monkeypatch.setenv("CVX_DEFER_NORM", "1")
    assert not route_seq_times(1 << 20, 512, "f16x3", 1 << 20).deferred


# ---------------------------------------------------------------- refusals: the host layer
def _rows(M=12, D=80, C=80):
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    return dict(x1=z(M, D), x0=z(M, D), cond=z(M, C), mask=torch.zeros(M, dtype=torch.bool), times=z(2), w=z(M, D))


def test_seq_offsets_refusals():
    from covomix_amd import ops
    host, n = ops.seq_offsets([0, 5, 5, 12], 12)
    assert host.dtype == torch.int32 and host.tolist() == [0, 5, 5, 12] and n == 3
    assert ops.seq_offsets([3, 9], 12)[1] == 1
    for bad in ([0], [], [0, 5, 4], [-1, 3], [0, 13], [0, 2.0], [0, True]):
        with pytest.raises(ValueError):
            ops.seq_offsets(bad, 12)
    with pytest.raises(ValueError):
        ops.seq_offsets(list(range(ops.SEQ_NORM_MAX_SEQS + 2)), 1 << 20)
    assert ops.seq_offsets(list(range(ops.SEQ_NORM_MAX_SEQS + 1)), 1 << 20)[1] == ops.SEQ_NORM_MAX_SEQS == 4096
    assert ops.masked_mse_tree_depth(1) == 9 and ops.masked_mse_tree_depth(256) == 9 and ops.masked_mse_tree_depth(257) == 10


def test_cfm_inputs_refusals():
    from covomix_amd import ops
    a = _rows()
    call = lambda **kw: ops.cfm_inputs(*[dict(a, **kw)[k] for k in ("x1", "x0", "cond", "mask", "times")], kw.get("seqs", [0, 5, 12]),
                                       kw.get("sigma", 0.0), dict(a, **kw)["w"])
    for kw in (dict(x0=torch.zeros(12, 76)), dict(cond=torch.zeros(11, 80)), dict(w=torch.zeros(12, 84)), dict(times=torch.zeros(3)),
               dict(sigma=-0.1), dict(sigma=1.5), dict(sigma=float("nan")), dict(seqs=[0, 5, 13]), dict(seqs=[0, 7, 5]),
               dict(x1=torch.zeros(12, 6), x0=torch.zeros(12, 6), w=torch.zeros(12, 6))):
        with pytest.raises(ValueError):
            call(**kw)
    for kw in (dict(x1=torch.zeros(12, 80, dtype=torch.float64)), dict(mask=torch.zeros(12)), dict(times=torch.zeros(2, dtype=torch.float64)),
               dict(x1=torch.zeros(80, 12).t())):
        with pytest.raises(TypeError):
            call(**kw)


def test_adarmsnorm_seq_and_masked_mse_refusals():
    from covomix_amd import ops
    x, out = torch.zeros(12, 64), torch.zeros(12, 64)
    g = torch.zeros(2, 64)
    for args in ((x, torch.zeros(3, 64), None, out, [0, 5, 12]), (x, g, torch.zeros(2, 32), out, [0, 5, 12]), (x, g, None, out, [0, 5, 13]),
                 (x, g, None, None, [0, 5, 12]), (x, g, None, torch.zeros(11, 64), [0, 5, 12]), (x, torch.zeros(2, 128)[:, ::2], None, out, [0, 5, 12]),
                 (x, torch.zeros(2, 66)[:, :64], None, out, [0, 5, 12]), (torch.zeros(12, 66), torch.zeros(2, 66), None, torch.zeros(12, 66), [0, 5, 12])):
        with pytest.raises(ValueError):
            ops.adarmsnorm_seq(*args)
    with pytest.raises(TypeError):
        ops.adarmsnorm_seq(x.double(), g, None, out, [0, 5, 12])
    p, m = torch.zeros(12, 80), torch.zeros(12, dtype=torch.bool)
    for args in ((p, torch.zeros(12, 76), m, [0, 12]), (p, p, torch.zeros(11, dtype=torch.bool), [0, 12]), (p, p, m, [0, 13]), (p, p, m, [5, 2])):
        with pytest.raises(ValueError):
            ops.masked_mse(*args)
    with pytest.raises(ValueError):
        ops.masked_mse(p, p, m, [0, 12], err_rows=torch.zeros(11))
    with pytest.raises(TypeError):
        ops.masked_mse(p, p, m.float(), [0, 12])


# ---------------------------------------------------------------- refusals: the facade
def _tiny_model():
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel
    shapes = syn.acoustic_param_shapes(dim=64, dim_cond=80, dim_emb=16, depth=2, heads=1, streams=1)
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed=0).items()}
    return CoVoMixModel.from_state_dict(sd)


def test_facade_refusals():
    from covomix_amd._lib import CovomixHipError
    from covomix_amd.conditional_model import CoVoMixModel
    model = _tiny_model()
    ids, mels = [torch.zeros(5, dtype=torch.int64), torch.zeros(7, dtype=torch.int64)], [torch.zeros(5, 80), torch.zeros(7, 80)]
    ok = dict(phoneme_ids=ids, mels=mels)
    for kw in (dict(phoneme_ids=[], mels=[]), dict(mels=mels[:1]), dict(cond_mels=mels[:1]), dict(masks=[torch.ones(5, dtype=torch.bool)]),
               dict(times=[0.5]), dict(cond_drop=[True]), dict(x0=[torch.zeros(5, 80)]),
               dict(phoneme_ids=[ids[0], torch.zeros(6, dtype=torch.int64)]), dict(mels=[mels[0], torch.zeros(7, 64)]),
               dict(cond_mels=[mels[0], torch.zeros(6, 80)]), dict(cond_mels=[torch.zeros(5, 160), torch.zeros(7, 160)]),
               dict(masks=[torch.ones(5, dtype=torch.bool), torch.ones(6, dtype=torch.bool)]), dict(masks=[torch.ones(5), torch.ones(7)]),
               dict(x0=[torch.zeros(5, 80), torch.zeros(7, 79)]), dict(times=[0.5, 1.5]), dict(times=[-0.01, 0.5]), dict(times=[0.5, float("nan")]),
               dict(sigma=2.0), dict(max_rows=0), dict(phoneme_ids=ids[0], mels=mels[0])):
        with pytest.raises(ValueError):
            model.flow_matching_loss(**dict(ok, **kw))
    # a mask without a True frame is not refused: the call gets as far as asking for the GPU (this model sits on the CPU)
    with pytest.raises(CovomixHipError):
        model.flow_matching_loss(ids, mels, masks=[torch.zeros(5, dtype=torch.bool), torch.zeros(7, dtype=torch.bool)], times=[0.0, 1.0], seed=0)
    t2s = CoVoMixModel({"token_emb.text.weight": torch.zeros(1, 1)})
    with pytest.raises(TypeError):
        t2s.flow_matching_loss(ids, mels)
    with pytest.raises(TypeError):
        t2s.synthesis_regression_duration(ids, mels, None, 0.7)
    for kw in (dict(times=[0.5]), dict(times=[0.5, 2.0]), dict(y0=[torch.zeros(5, 80)]), dict(y0=[torch.zeros(5, 80), torch.zeros(7, 8)])):
        with pytest.raises(ValueError):
            model.synthesis_regression_duration(ids, mels, None, 0.7, **kw)
    with pytest.raises(ValueError):
        model.synthesis_regression_duration(ids, [mels[0], torch.zeros(6, 80)], None, 0.7)
    # the null branch doubles the sequences of the one evaluation: 2049 guided utterances are refused by the facade itself, by name
    many_ids, many_mels = [torch.zeros(1, dtype=torch.int64)] * 2049, [torch.zeros(1, 80)] * 2049
    with pytest.raises(ValueError, match="at most 2048 under guidance"):
        model.synthesis_regression_duration(many_ids, many_mels, None, 0.7, times=[0.5] * 2049)
    with pytest.raises(CovomixHipError):         # at scale 1 the same call passes every check (this model sits on the CPU)
        model.synthesis_regression_duration(many_ids, many_mels, None, 1.0, times=[0.5] * 2049)
    with pytest.raises(ValueError, match="at most 4096"):
        model.synthesis_regression_duration(many_ids * 2, many_mels * 2, None, 1.0, times=[0.5] * 4098)


# ---------------------------------------------------------------- header, binding, code objects
ENTRIES = ("cvx_adarmsnorm_seq_f32", "cvx_cfm_inputs_f32", "cvx_masked_mse_f32")


def test_header_binding_and_version():
    import ctypes as C
    from covomix_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "covomix_hip.h")).read()
    assert "Still ABI 113: three symbols and one constant added" in hdr
    assert re.search(r"#define\s+CVX_ABI_VERSION\s+113\b", hdr) and _lib.ABI_VERSION == 113
    assert re.search(r"#define\s+CVX_SEQ_NORM_MAX_SEQS\s+4096\b", hdr) and _lib.SEQ_NORM_MAX_SEQS == ops.SEQ_NORM_MAX_SEQS == 4096
    lib = _lib.load()
    assert lib.cvx_version() == 113
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args[-1] is C.c_void_p and hasattr(lib, name)
        proto = re.search(name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert len(args) == proto.count(",") + 1, name
    assert os.path.isfile(os.path.join(ROOT, "neurips2024-covomix_amd", "csrc", "flow_loss.hip"))


def test_new_kernels_use_no_private_segment_and_fit_lds():
    from covomix_amd import _lib
    from test_attention_form_d import _gfx950_kernel_descriptors
    kds = {k: v for k, v in _gfx950_kernel_descriptors(_lib.LIB_PATH).items()
           if any(s in k for s in ("adanorm_seq", "cfm_inputs_kernel", "cfm_row_mse_kernel", "cfm_seq_loss_kernel"))}
    assert len(kds) == 7, sorted(kds)            # three in-register norm instances, the generic one, inputs, row errors, sequence sums
    for name, (group, private, vgprs) in kds.items():
        print(f"FIGURE {name[:70]}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
        assert private == 0 and group <= 64 and vgprs <= 128, (name, group, private, vgprs)
    # the names stay clear of the substrings other tests count kernels by
    for name in kds:
        for taken in ("dtw", "rk_err_", "rk_stage_kernel", "t2s_prefill", "attention_f16x3_kernel", "gemm_f16x3_p8s_kernel", "beam_"):
            assert taken not in name, (name, taken)


# ---------------------------------------------------------------- the tool
def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("eval_flow_loss", os.path.join(ROOT, "tools", "eval_flow_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_parser():
    tool = _tool()
    ap = tool.build_parser()
    a = ap.parse_args(["--ckpt", "c", "--mel_dir", "m", "--token_dir", "t", "--json", "o"])
    assert (a.seed, a.draws, a.times, a.precision, a.max_rows, a.cond_dir) == (0, 1, None, None, 8192, None)
    a = ap.parse_args(["--ckpt", "c", "--mel_dir", "m", "--token_dir", "t", "--json", "o", "--times", "0,0.5,1", "--draws", "3", "--seed", "9",
                       "--precision", "fp32", "--max_rows", "100", "--cond_dir", "k"])
    assert a.times == [0.0, 0.5, 1.0] and (a.draws, a.seed, a.precision, a.max_rows, a.cond_dir) == (3, 9, "fp32", 100, "k")
    for bad in (["--times", "0,2"], ["--times", "x"], ["--times", ""], ["--draws", "0"], ["--max_rows", "-1"], ["--precision", "bf16"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--ckpt", "c", "--mel_dir", "m", "--token_dir", "t", "--json", "o"] + bad)
    with pytest.raises(SystemExit):
        ap.parse_args(["--mel_dir", "m", "--token_dir", "t", "--json", "o"])
    assert "random-weight" in tool.NOTE and "random-weight" in tool.__doc__


def test_tool_pairs_by_stem_and_lists_the_rest(tmp_path):
    tool = _tool()
    mel, tok, cond = tmp_path / "mel", tmp_path / "tok", tmp_path / "cond"
    for d in (mel, tok, cond):
        d.mkdir()
    for s in ("a", "b", "c"):
        np.save(mel / f"{s}.mel.npy", np.zeros((80, 4), np.float32))
    for s in ("b", "c", "d"):
        np.save(tok / f"{s}.semantic.npy", np.zeros(4, np.int64))
    for s in ("c", "e"):
        np.save(cond / f"{s}.mel.npy", np.zeros((80, 4), np.float32))
    (mel / "notes.txt").write_text("x")
    pairs, missing = tool.pair_by_stem(str(mel), str(tok))
    assert [p[0] for p in pairs] == ["b", "c"] and all(p[3] is None for p in pairs)
    assert missing == dict(no_tokens=["a"], no_mel=["d"])
    pairs, missing = tool.pair_by_stem(str(mel), str(tok), str(cond))
    assert [p[0] for p in pairs] == ["c"] and pairs[0][3].endswith("c.mel.npy")
    assert missing == dict(no_tokens=["a"], no_mel=["d"], no_cond=["b"], cond_only=["e"])
    mels, toks, conds = tool.load(pairs)
    assert mels[0].shape == (4, 80) and toks[0].dtype == torch.int64 and conds[0].shape == (4, 80)
