"""GPU: the text2semantic sampling controls through the C ABI - the logit filters (top-k with any k, top-p; reference
text2semantic.py:118-132) in the stand-alone sampling entry and in every decode schedule, classifier-free guidance in the
continuously refilled slots (generate_many(cond_scale=)), the descriptors the library refuses, the facade and the CLI flags.
Kept sets and tokens are compared EXACTLY (tests/golden/t2s_filters.npz holds the reference's own masks; the restatement of
tests/t2s_filter_restated.py is pinned against them on the CPU, tests/test_t2s_filters.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import t2s_filter_restated as rs
from test_t2s_filters import (BLOCKS, DECODE_FILTERS, DECODE_STEPS, TEMPS, decode_uniforms, fixture_block, fixture_uniforms, load_small)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = 1.5
EINVAL = -22


@pytest.fixture(scope="module")
def decoders():
    from covomix_amd.t2s import TextToSemanticDecoder
    out = {}
    for name in ("cosingle_small", "comix_small"):
        g, sd = load_small(name)
        out[name] = (g, TextToSemanticDecoder(sd, torch.device(DEV), max_length=256))
    return out


# ---------------------------------------------------------------- cvx_t2s_sample_f32 on the fixture
@pytest.mark.parametrize("V", BLOCKS)
def test_sample_entry_kept_masks_and_tokens_on_the_fixture(V):
    """Every row and setting: the kept mask equals the reference's (V = 503: whole 4-vectors over the padded tail; V = 1024: the LDS
    limit); the token equals the fp64 argmax of kept ? l / T + gumbel(u) : -inf wherever that score's top-2 margin exceeds DELTA
    (at most 2 % of the rows may lie inside it; in fp64 none does, tests/test_t2s_filters.py); all rows in one launch == row by row."""
    from covomix_amd import ops
    logits, kept, sets = fixture_block(V)
    u = fixture_uniforms(V, logits.shape[0])
    lg, ug = logits.to(DEV), u.to(DEV)
    n = inside = 0
    for i, (name, mode, k, thres) in enumerate(sets):
        for T in TEMPS:
            tok, km = ops.t2s_sample(lg, ug, mode, k, thres, T, return_kept=True)
            assert torch.equal(km.cpu().bool(), kept[i]), (V, name, T, int((km.cpu().bool() != kept[i]).sum()))
            score = rs.score_of(logits, u, kept[i], T)
            ok = rs.margin_ok(score)
            assert torch.equal(tok.cpu()[ok], score.argmax(dim=-1)[ok]), (V, name, T)
            n += ok.numel()
            inside += int((~ok).sum())
            assert torch.equal(ops.t2s_sample(lg, ug, mode, k, thres, T), tok)              # without the mask output: the same tokens
        rows = [ops.t2s_sample(lg[r:r + 1].clone(), ug[r:r + 1].clone(), mode, k, thres, TEMPS[-1], return_kept=True) for r in range(lg.shape[0])]
        assert torch.equal(torch.cat([r[0] for r in rows]), tok) and torch.equal(torch.cat([r[1] for r in rows]), km), (V, name)
    print(V, "rows inside the margin:", inside, "of", n)
    assert inside <= 0.02 * n


def test_sample_entry_ties():
    """top-k keeps every entry that equals the k-th largest (rank counting: fewer than k logits are larger - the rule of the header,
    unchanged from the decode before this entry point existed); top-p orders equal logits by index"""
    from covomix_amd import ops
    l = torch.tensor([[0.0, 2.0, 2.0, 2.0, -1.0]], device=DEV)
    u = torch.full_like(l, 0.5)
    p = float(torch.softmax(l.double(), -1)[0, 1])
    tok, km = ops.t2s_sample(l, u, rs.TOP_K, 2, 0.0, 1.0, return_kept=True)
    assert km.tolist() == [[0, 1, 1, 1, 0]] and tok.tolist() == [1]
    assert ops.t2s_sample(l, u, rs.TOP_K, 4, 0.0, 1.0, return_kept=True)[1].tolist() == [[1, 1, 1, 1, 0]]
    assert ops.t2s_sample(l, u, rs.TOP_P, 0, p + 1e-3, 1.0, return_kept=True)[1].tolist() == [[0, 1, 1, 0, 0]]
    assert ops.t2s_sample(l, u, rs.TOP_P, 0, p - 1e-3, 1.0, return_kept=True)[1].tolist() == [[0, 1, 0, 0, 0]]


# ---------------------------------------------------------------- decode with a filter
def _texts(g, n, seed):
    """n texts of different length cut from the golden one"""
    src = torch.from_numpy(g["source_ids"])
    gen = torch.Generator().manual_seed(seed)
    L = src.shape[1]
    out = []
    for i in range(n):
        a = int(torch.randint(0, max(1, L // 2), (1,), generator=gen))
        e = int(torch.randint(a + 3, L + 1, (1,), generator=gen))
        out.append(src[:, a:e] if i % 5 else torch.cat((src, src[:, : 1 + i % 7]), dim=1))
    return out


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
@pytest.mark.parametrize("filt", list(DECODE_FILTERS))
def test_decode_with_a_filter(decoders, name, filt):
    g, model = decoders[name]
    fn, kw = DECODE_FILTERS[filt]
    src = torch.from_numpy(g["source_ids"])
    S, V = g["uniforms"].shape[1], g["uniforms"].shape[-1]
    mode, k, thres = rs.setting(fn, V, **kw)
    uni = decode_uniforms(S, V)
    flat, streams, logits = model.generate(src, uniforms=uni, collect_logits=True, filter_logits_fn=fn, filter_fn_kwargs=kw)
    L = streams.shape[1]
    tokens, decidable = rs.restated_choice(logits.cpu(), uni[:L], 1.0, mode, k, thres)      # on the GPU's own logits of every step
    got = streams.cpu().T
    print(name, filt, "steps", L, "undecidable", int((~decidable).sum()))
    assert torch.equal(got[decidable], tokens[decidable])
    assert int((~decidable).sum()) <= 0.05 * decidable.numel()
    kept = rs.kept_mask(logits.cpu(), mode, k, thres)
    assert bool(kept.gather(-1, got[..., None]).all()), "a sampled token outside the kept set"
    replay, rstreams = model.generate(src, uniforms=uni, filter_logits_fn=fn, filter_fn_kwargs=kw, return_streams=True)   # graph replay
    assert torch.equal(replay, flat) and torch.equal(rstreams, streams)
    default = model.generate(src, uniforms=uni, return_streams=True)[1]
    n = min(default.shape[1], L)
    assert not torch.equal(default[:, :n], streams[:, :n]), "the filter setting did not arrive"
    srcs = _texts(g, 10, seed=3)
    unis = [decode_uniforms(S, V, salt=1 + i) for i in range(len(srcs))]
    alone = [model.generate(s_, uniforms=u_, return_streams=True, filter_logits_fn=fn, filter_fn_kwargs=kw) for s_, u_ in zip(srcs, unis)]
    batch = model.generate_batch(srcs, unis, filter_logits_fn=fn, filter_fn_kwargs=kw)
    many = model.generate_many(srcs, unis, slots=8, filter_logits_fn=fn, filter_fn_kwargs=kw)
    for j, a in enumerate(alone):
        assert torch.equal(batch[j][0], a[0]) and torch.equal(batch[j][1], a[1]), (name, filt, "batch", j)
        assert torch.equal(many[j][0], a[0].cpu()) and torch.equal(many[j][1], a[1].cpu()), (name, filt, "many", j)


# ---------------------------------------------------------------- guided continuous batching
N_GUIDED, GOLD_AT = 20, 10


@pytest.fixture(scope="module")
def guided(decoders):
    """20 utterances of varied text and limits (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK, ...: refills on the first, last and middle step
    of a graph replay), the utterance of t2s_cosingle_small_cfg.npz in the middle, and every one's guided decode ALONE"""
    from covomix_amd.t2s import CHUNK
    g, model = decoders["cosingle_small"]
    gold = np.load(os.path.join(GOLDEN, "t2s_cosingle_small_cfg.npz"))
    assert float(gold["cond_scale"]) == CFG
    V = g["uniforms"].shape[-1]
    srcs = _texts(g, N_GUIDED, seed=5)
    unis = [decode_uniforms(1, V, salt=100 + i) for i in range(N_GUIDED)]
    gen = torch.Generator().manual_seed(9)
    limits = [1, CHUNK, CHUNK + 1, CHUNK - 1, 2 * CHUNK, 2, 3 * CHUNK - 1] + torch.randint(3, DECODE_STEPS + 1, (N_GUIDED - 7,), generator=gen).tolist()
    gu = torch.from_numpy(gold["uniforms"])[:, :, 0, :]
    srcs[GOLD_AT], unis[GOLD_AT], limits[GOLD_AT] = torch.from_numpy(gold["source_ids"]), torch.cat((gu, unis[GOLD_AT][gu.shape[0]:])), gu.shape[0]
    alone = [model.generate(s_, uniforms=u_[:l_], return_streams=True, cond_scale=CFG) for s_, u_, l_ in zip(srcs, unis, limits)]
    assert torch.equal(alone[GOLD_AT][0].cpu(), torch.from_numpy(gold["tokens"]))
    return model, gold, srcs, unis, limits, alone


@pytest.mark.parametrize("slots", [2, 8, 16])
def test_guided_continuous_batching_equals_alone(guided, slots):
    """generate_many(cond_scale = 1.5): slot pairs refilled on the device with dialogue record pairs.  More utterances than pairs;
    every utterance gets exactly its tokens alone, the golden one the reference's; both endings occur and every pair is used."""
    model, gold, srcs, unis, limits, alone = guided
    done = []
    res = model.generate_many(srcs, unis, slots=slots, limits=limits, cond_scale=CFG, on_done=lambda j, r: done.append(j))
    assert sorted(done) == list(range(N_GUIDED))
    rec = model.last_records
    assert len(rec) == N_GUIDED
    for j in range(N_GUIDED):
        assert torch.equal(res[j][0], alone[j][0].cpu()) and torch.equal(res[j][1], alone[j][1].cpu()), (slots, j, rec[j])
        assert rec[j][4] == alone[j][1].shape[1]
    assert torch.equal(res[GOLD_AT][0], torch.from_numpy(gold["tokens"]))
    by_eos = sum(1 for r in rec if r[3] == 2)
    by_limit = sum(1 for r in rec if r[3] == 3)
    used = {r[5] for r in rec}
    print(f"{slots} slots: {by_eos} ended by their eos, {by_limit} by their limit; pairs used: {len(used)}")
    assert by_eos + by_limit == N_GUIDED and by_eos > 0 and by_limit > 0
    assert used == set(range(0, slots, 2))


def test_guided_continuous_batching_with_idle_pairs(guided):
    """fewer utterances than slot pairs: 3 utterances on 8 slots (4 pairs, one never used)"""
    model, gold, srcs, unis, limits, alone = guided
    pick = [GOLD_AT, 0, 4]
    res = model.generate_many([srcs[j] for j in pick], [unis[j] for j in pick], slots=16, limits=[limits[j] for j in pick], cond_scale=CFG)
    for r, j in zip(res, pick):
        assert torch.equal(r[0], alone[j][0].cpu()) and torch.equal(r[1], alone[j][1].cpu()), j
    assert {r[5] for r in model.last_records} == {0, 2, 4}
    state = model.buf["state"].tolist()
    assert all(state[s][0] == model.max_length for s in range(8)), "every slot idles once the queue is drained"


def test_guided_continuous_batching_with_top_p(guided):
    model, gold, srcs, unis, limits, alone = guided
    kw = dict(cond_scale=CFG, filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.9})
    pick = list(range(3, 10))
    one = [model.generate(srcs[j], uniforms=unis[j][: limits[j]], return_streams=True, **kw) for j in pick]
    res = model.generate_many([srcs[j] for j in pick], [unis[j] for j in pick], slots=4, limits=[limits[j] for j in pick], **kw)
    for r, a in zip(res, one):
        assert torch.equal(r[0], a[0].cpu()) and torch.equal(r[1], a[1].cpu())
    assert any(not torch.equal(a[1], alone[j][1]) for a, j in zip(one, pick)), "top_p did not arrive in the guided decode"


def test_guidance_on_a_two_output_model_is_refused(decoders):
    g, model = decoders["comix_small"]
    src = torch.from_numpy(g["source_ids"])
    with pytest.raises(NotImplementedError):
        model.generate_many([src, src], cond_scale=CFG, max_length=8)
    with pytest.raises(NotImplementedError):
        model.generate(src, cond_scale=CFG, max_length=8)


# ---------------------------------------------------------------- descriptors the library refuses
def test_abi_refuses_bad_sampling_descriptors(decoders):
    """CVX_EINVAL and nothing launched (the slot records keep the pattern written before the call)"""
    from covomix_amd import _lib, ops
    g, model = decoders["cosingle_small"]
    lib = _lib.load()
    V = model.d["vocab"]
    model._ensure(8, 8, 16)
    sentinel = torch.full_like(model.buf["state"], 5)          # position 5 of 256: a launch would advance it
    model.buf["state"].copy_(sentinel)

    def call(**edit):
        dec = model._descriptor(1.0, edit.pop("batch", 8), edit.pop("cfg_scale", 1.0), edit.pop("queue", False), None, edit.pop("nd", 0))
        for name, v in edit.items():
            setattr(dec, name, v)
        rc = lib.cvx_t2s_decode_steps(C.byref(dec), 1, ops._stream())
        torch.cuda.synchronize()
        return rc

    assert call(cfg_scale=CFG, queue=True, nd=7) == EINVAL                  # an odd number of dialogue records under guidance
    assert call(cfg_scale=CFG, queue=True, nd=0) == EINVAL
    assert call(top_k=0) == EINVAL and call(top_k=V + 1) == EINVAL and call(top_k=-3) == EINVAL
    assert call(filter_mode=2) == EINVAL and call(filter_mode=-1) == EINVAL
    assert call(filter_mode=1, top_p=0.0) == EINVAL and call(filter_mode=1, top_p=1.0) == EINVAL
    assert torch.equal(model.buf["state"], sentinel)
    lg = torch.zeros(2, V, device=DEV)
    tok = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    for mode, k, thres in ((0, 0, 0.0), (0, V + 1, 0.0), (3, 1, 0.5), (1, 0, 1.0)):
        assert lib.cvx_t2s_sample_f32(lg.data_ptr(), lg.data_ptr(), 2, V, mode, k, thres, 1.0, tok.data_ptr(), None, ops._stream()) == EINVAL
    torch.cuda.synchronize()
    assert tok.tolist() == [-7, -7]
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- facade and CLI
def test_facade_guided_list_equals_one_by_one(guided):
    from covomix_amd.conditional_model import CoVoMixModel
    _, gold, srcs, unis, limits, _ = guided
    _, sd = load_small("cosingle_small")
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval().to(DEV)
    pick = [GOLD_AT, 1, 2, 7, 8]
    ids, us = [srcs[j] for j in pick], [unis[j] for j in pick]
    for kw in ({}, {"filter_logits_fn": "top_p", "filter_fn_kwargs": {"thres": 0.9}}):
        many = m.synthesis_sample_text2semantic(ids, cond_scale=CFG, uniforms=us, slots=4, **kw)
        for j, (i_, u_) in enumerate(zip(ids, us)):
            assert torch.equal(many[j], m.synthesis_sample_text2semantic(i_, cond_scale=CFG, uniforms=u_, **kw)), (kw, j)
    # (the golden utterance decodes past its recorded draws here, up to the eos the reference sampled with them)
    first = m.synthesis_sample_text2semantic(ids, cond_scale=CFG, uniforms=us, slots=4)[0]
    assert torch.equal(first[: gold["tokens"].shape[0]], torch.from_numpy(gold["tokens"]))


def test_cli_passes_the_sampling_flags(tmp_path, monkeypatch):
    """the five --t2s_* flags reach CoVoMixModel.synthesis_sample_text2semantic as keywords; without them none that changes behaviour"""
    import covomix_amd.synthetic as syn
    from covomix_amd import generation
    from test_generation_gpu import _write_fixture
    tmp = str(tmp_path)
    _write_fixture(tmp, "vomix")
    shapes = syn.t2s_param_shapes(two_output=True, dim=64, dim_target=128, source_depth=2, target_depth=2, heads=1, num_text=200)
    tsd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=0).items()}
    torch.save({"state_dict": {"cfm_wrapper.model." + k: v for k, v in tsd.items()},
                "hyper_parameters": {"text2semantic": True, "text2semantic_two_output": True}}, os.path.join(tmp, "t2s.ckpt"))
    tdir, pdir = os.path.join(tmp, "text"), os.path.join(tmp, "prompt")
    os.makedirs(tdir); os.makedirs(pdir)
    rng = np.random.RandomState(1)
    for suf in ("_1", "_2"):
        np.save(os.path.join(pdir, f"dlg_a{suf}.hubert_code.npy"), rng.randint(0, 510, size=20))
        np.save(os.path.join(pdir, f"dlg_a{suf}.mel.npy"), (rng.randn(80, 20) * 2 - 6).astype(np.float32))
    np.save(os.path.join(tdir, "dlg_a.text_ids.npy"), rng.randint(1, 199, size=(1, 9)).astype(np.int64))
    real = generation.CoVoMixModel.synthesis_sample_text2semantic
    seen = []

    def spy(self, ids, **kw):
        seen.append({k: v for k, v in kw.items() if k not in ("uniforms", "slots")})
        return real(self, ids, uniforms=kw["uniforms"], max_length=12, **{k: v for k, v in kw.items() if k.startswith("filter") or k == "temprature"})
    monkeypatch.setattr(generation.CoVoMixModel, "synthesis_sample_text2semantic", spy)
    base = ["--t2s_ckpt", os.path.join(tmp, "t2s.ckpt"), "--acous_ckpt", os.path.join(tmp, "acous.ckpt"),
            "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"), "--text_dir", tdir, "--prompt_dir", pdir, "--mode", "covomix"]
    with pytest.warns(UserWarning, match="EMA"):
        assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, "o1")]) == 1
        assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, "o2"), "--pipeline", "off", "--t2s_temperature", "0.7", "--t2s_cond_scale", "1.5",
                                            "--t2s_filter", "top_k", "--t2s_filter_thres", "0.3", "--t2s_top_k", "9"]) == 1
        assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, "o3"), "--pipeline", "serial", "--t2s_filter", "top_p",
                                            "--t2s_filter_thres", "0.8"]) == 1
    assert seen[0] == {}
    assert seen[1] == dict(temprature=0.7, cond_scale=1.5, filter_logits_fn="top_k", filter_fn_kwargs={"thres": 0.3, "k": 9})
    assert seen[2] == dict(filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.8})
