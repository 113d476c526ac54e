"""GPU: text2semantic token log-probabilities, teacher-forced scoring and best-of-N.

  1. cvx_t2s_logprob_f32 (the log-prob epilogue alone) against fp64 log_softmax on the rows of tests/t2s_logprob_restated.py;
  2. score_many (forced dialogues) against the fp64 oracle's teacher-forced logits, with and without guidance;
  3. the log-probs of a SAMPLED sequence equal the forced score of the same tokens BIT FOR BIT, in every decode schedule;
  4. forced scores do not depend on the slots, the refills or on sampled neighbours in the same queue;
  5. with return_logprobs off nothing moves (tokens, graph cache keys, ABI version);
  6. the facade (best_of, score_text2semantic) and the CLI flag;
  7. the descriptors cvx_t2s_decode_steps_scored refuses.
The fixtures are the committed cosingle_small / comix_small models with max_length = 40."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import t2s_logprob_restated as rs
from test_t2s_filters import decode_uniforms, load_small

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = 1.5
EINVAL = -22
MAX_LEN = 40


@pytest.fixture(scope="module")
def decoders():
    from covomix_amd.t2s import TextToSemanticDecoder
    out = {}
    for name in ("cosingle_small", "comix_small"):
        g, sd = load_small(name)
        out[name] = (g, sd, TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN))
    return out


def _golden(g):
    """(source ids, uniforms [steps, S, V], streams [S, L]) of a golden file, cut to MAX_LEN steps"""
    return (torch.from_numpy(g["source_ids"]), torch.from_numpy(g["uniforms"])[:MAX_LEN, :, 0, :],
            torch.from_numpy(g["streams"])[0, :, :MAX_LEN])


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


# ---------------------------------------------------------------- 1. the epilogue alone
@pytest.mark.parametrize("V", rs.VOCABS)
def test_logprob_entry_against_fp64(V):
    from covomix_amd import ops
    lg, tk = rs.rows_for(V)
    ref = rs.reference(lg, tk)
    for order in rs.SUMS:                        # the inputs are decidable: fp32 arithmetic in any summation order meets the bound
        assert bool(((rs.restated(lg, tk, order).double() - ref).abs() <= rs.bound(ref)).all()), (V, order)
    got = ops.t2s_logprob(lg.to(DEV), tk.to(DEV)).cpu()
    u = rs.ulps(got, ref)
    print(f"V = {V}: largest error {float(u.max()):.2f} units of 2^-24 (1 + |lp|) over {lg.shape[0]} rows")
    assert bool(torch.isfinite(got).all())
    assert bool(((got.double() - ref).abs() <= rs.bound(ref)).all()), (V, float(u.max()))
    # a function of the row alone: row by row == all rows in one launch
    one = torch.cat([ops.t2s_logprob(lg[r:r + 1].to(DEV), tk[r:r + 1].to(DEV)) for r in range(0, lg.shape[0], 7)]).cpu()
    assert torch.equal(one, got[0::7])


def test_logprob_entry_refusals():
    from covomix_amd import _lib, ops
    lib = _lib.load()
    lg = torch.zeros(2, 1100, device=DEV)
    tk = torch.zeros(2, dtype=torch.int64, device=DEV)
    out = torch.full((2,), -7.0, device=DEV)
    for rows, V in ((2, 0), (2, -1), (2, 1025), (-1, 16)):
        assert lib.cvx_t2s_logprob_f32(lg.data_ptr(), tk.data_ptr(), rows, V, out.data_ptr(), ops._stream()) == EINVAL, (rows, V)
    assert lib.cvx_t2s_logprob_f32(None, tk.data_ptr(), 2, 16, out.data_ptr(), ops._stream()) == EINVAL
    assert lib.cvx_t2s_logprob_f32(lg.data_ptr(), tk.data_ptr(), 2, 16, None, ops._stream()) == EINVAL
    torch.cuda.synchronize()
    assert out.tolist() == [-7.0, -7.0]
    assert lib.cvx_t2s_logprob_f32(lg.data_ptr(), tk.data_ptr(), 0, 16, out.data_ptr(), ops._stream()) == 0      # no rows: nothing to do
    torch.cuda.synchronize()
    assert out.tolist() == [-7.0, -7.0]
    tk[1] = 16                                   # a token outside [0, V) indexes nothing: NaN
    assert lib.cvx_t2s_logprob_f32(lg.data_ptr(), tk.data_ptr(), 2, 16, out.data_ptr(), ops._stream()) == 0
    torch.cuda.synchronize()
    assert out[0].item() == pytest.approx(-np.log(16.0), rel=1e-6) and bool(torch.isnan(out[1]))


# ---------------------------------------------------------------- 2. forced scoring against the oracle
def _oracle_check(sd, src, streams, lp, cond_scale, what):
    """per position: |lp - lp64| <= 2 LONG_LOGIT_TOL ||logits64[pos, s]||_2 + 256 * 2^-24 (1 + |lp64|) - a perturbation d of a row of logits moves
    a log-prob by at most 2 ||d||_inf <= 2 ||d||_2, and LONG_LOGIT_TOL is the project's bound on ||d||_2 / ||logits||_2"""
    import t2s_oracle as orc
    lg64 = orc.teacher_forced_logits(sd, src, streams, cond_scale=cond_scale, dtype=torch.float64)        # [L, S, V]
    lp64 = torch.log_softmax(lg64, dim=-1).gather(-1, streams.T[..., None])[..., 0].T                        # [S, L]
    bound = 2 * orc.LONG_LOGIT_TOL * lg64.norm(dim=-1).T + rs.bound(lp64)
    err = (lp.double() - lp64).abs()
    print(f"{what}: largest |lp - lp64| {float(err.max()):.3e}, largest error / bound {float((err / bound).max()):.3f}, "
          f"mean lp {float(lp64.mean()):.3f}")
    assert lp.shape == streams.shape and lp.dtype == torch.float32
    assert bool((err <= bound).all()), (what, float((err / bound).max()))


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_forced_scoring_against_the_oracle(decoders, name):
    g, sd, model = decoders[name]
    src, _, streams = _golden(g)
    lp = model.score_many([src], [streams])[0]
    _oracle_check(sd, src, streams, lp, 1.0, name)


def test_forced_scoring_under_guidance_against_the_oracle(decoders):
    _, sd, model = decoders["cosingle_small"]
    gold = np.load(os.path.join(GOLDEN, "t2s_cosingle_small_cfg.npz"))
    assert float(gold["cond_scale"]) == CFG
    src, streams = torch.from_numpy(gold["source_ids"]), torch.from_numpy(gold["streams"])[0, :, :MAX_LEN]
    lp = model.score_many([src], [streams], cond_scale=CFG)[0]
    _oracle_check(sd, src, streams, lp, CFG, "cosingle_small, cond_scale 1.5")
    plain = model.score_many([src], [streams])[0]
    assert not torch.equal(plain, lp), "the guidance did not arrive in the forced decode"


# ---------------------------------------------------------------- 3. sampled log-probs == forced scores, bit for bit
@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_sampled_logprobs_equal_the_forced_score(decoders, name):
    g, sd, model = decoders[name]
    src, uni, gold_streams = _golden(g)
    S, V = uni.shape[1], uni.shape[2]
    flat, streams, lp = model.generate(src, uniforms=uni, return_logprobs=True)
    assert torch.equal(streams.cpu(), gold_streams[:, :streams.shape[1]]) and lp.shape == streams.shape and lp.dtype == torch.float32
    assert bool((lp <= 0).all()) and bool(torch.isfinite(lp).all())
    assert torch.equal(model.score_many([src], [streams])[0], lp.cpu())
    srcs = _texts(g, 5, seed=3)
    unis = [decode_uniforms(S, V, salt=1 + i) for i in range(5)]
    batch = model.generate_batch(srcs, unis, return_logprobs=True)
    many = model.generate_many(srcs, unis, slots=2, return_logprobs=True)            # 5 utterances through 2 slots: refills
    plain = model.generate_many(srcs, unis, slots=2)
    scored = model.score_many(srcs, [r[1] for r in many], slots=4)
    for j in range(5):
        assert len(batch[j]) == 3 and len(many[j]) == 3 and len(plain[j]) == 2
        assert torch.equal(many[j][0], plain[j][0]) and torch.equal(many[j][1], plain[j][1]), "the log-prob epilogue changed the tokens"
        assert torch.equal(batch[j][1].cpu(), many[j][1]) and torch.equal(batch[j][2].cpu(), many[j][2]), (name, j)
        assert torch.equal(scored[j], many[j][2]), (name, j)
    kw = dict(filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.9})
    one = model.generate(srcs[0], uniforms=unis[0], return_logprobs=True, **kw)
    tp = model.generate_many(srcs, unis, slots=2, return_logprobs=True, **kw)
    assert torch.equal(one[1].cpu(), tp[0][1]) and torch.equal(one[2].cpu(), tp[0][2])
    assert any(not torch.equal(a[1], b[1]) for a, b in zip(tp, many)), "top_p did not arrive"
    for j, s_ in enumerate(model.score_many(srcs, [r[1] for r in tp], slots=2)):
        assert torch.equal(s_, tp[j][2]), (name, "top_p", j)


def test_sampled_logprobs_equal_the_forced_score_under_guidance(decoders):
    g, sd, model = decoders["cosingle_small"]
    V = model.d["vocab"]
    srcs = _texts(g, 3, seed=5)
    unis = [decode_uniforms(1, V, salt=100 + i) for i in range(3)]
    many = model.generate_many(srcs, unis, slots=4, cond_scale=CFG, return_logprobs=True)     # 3 utterances through 2 slot pairs
    alone = [model.generate(s_, uniforms=u_, cond_scale=CFG, return_logprobs=True) for s_, u_ in zip(srcs, unis)]
    scored = model.score_many(srcs, [r[1] for r in many], cond_scale=CFG, slots=4)
    for j in range(3):
        assert torch.equal(alone[j][1].cpu(), many[j][1]) and torch.equal(alone[j][2].cpu(), many[j][2]), j
        assert torch.equal(scored[j], many[j][2]), j
    assert not torch.equal(model.score_many(srcs[:1], [many[0][1]])[0], many[0][2])


# ---------------------------------------------------------------- 4. independence of the launch shape
LENGTHS = [1, 2, 7, 16, 17, 33, 40, 15, 32]


def _targets(S, V, seed):
    gen = torch.Generator().manual_seed(seed)
    tg = [torch.randint(0, V, (S, L), generator=gen) for L in LENGTHS]
    tg[3][0, 2] = V - 1                              # an eos in the middle of a target: it ends nothing
    return tg


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_forced_scores_do_not_depend_on_the_launch_shape(decoders, name):
    g, sd, model = decoders[name]
    S, V = model.d["streams"], model.d["vocab"]
    srcs, tg = _texts(g, len(LENGTHS), seed=11), _targets(S, V, 21)
    ref = model.score_many(srcs, tg, slots=1)
    assert [tuple(r.shape) for r in ref] == [(S, L) for L in LENGTHS]
    assert all(rec[3] == 3 and rec[4] == L for rec, L in zip(model.last_records, LENGTHS)), "a forced dialogue ends at its limit only"
    for slots in (2, 4, 8, 16):
        got = model.score_many(srcs, tg, slots=slots)
        for j in range(len(LENGTHS)):
            assert torch.equal(got[j], ref[j]), (name, slots, j)
    # forced and sampled dialogues in ONE queue: every second dialogue is sampled
    ssrc = _texts(g, 4, seed=31)
    suni = [decode_uniforms(S, V, salt=50 + i) for i in range(4)]
    alone = model.generate_many(ssrc, suni, slots=4, return_logprobs=True)
    sources, forced, unis, where = [], [], [], []
    for j in range(len(LENGTHS)):
        sources.append(srcs[j]); forced.append(tg[j]); unis.append(None); where.append(("f", j))
        if j < 4:
            sources.append(ssrc[j]); forced.append(None); unis.append(suni[j]); where.append(("s", j))
    mixed = model.generate_many(sources, unis, slots=4, return_logprobs=True, forced=forced)
    for r, (kind, j) in zip(mixed, where):
        if kind == "f":
            assert torch.equal(r[1], tg[j]) and torch.equal(r[2], ref[j]), (name, "forced", j)
        else:
            assert torch.equal(r[0], alone[j][0]) and torch.equal(r[1], alone[j][1]) and torch.equal(r[2], alone[j][2]), (name, "sampled", j)


def test_forced_slot_record_without_a_queue(decoders):
    """flag bit 1 of the SLOT record is honoured without a queue: the slot scores its token row, ends at its limit and idles"""
    g, sd, model = decoders["comix_small"]
    src, _, streams = _golden(g)
    L = 9
    want = model.score_many([src], [streams[:, :L]])[0]
    model._ensure(1, 1, 16, True)
    ctx = model._contexts([src])
    model.buf["tokens"][0, :, :L].copy_(streams[:, :L].to(DEV))
    model.buf["logprobs"].fill_(7.0)
    model.buf["x"][:1].copy_(model.start[None, :])
    model.buf["state"].copy_(model._slot_records(ctx, limit=L, flags=2))
    model._run_steps(1.0, 1, L + 3, scored=True)
    torch.cuda.synchronize()
    assert torch.equal(model.buf["logprobs"][0, :, :L].cpu(), want)
    assert bool((model.buf["logprobs"][0, :, L:] == 7.0).all()), "steps behind the limit wrote nothing"
    assert model.buf["state"][0].tolist()[:3] == [MAX_LEN, 1, L]
    assert torch.equal(model.buf["tokens"][0, :, :L].cpu(), streams[:, :L])
    # cvx_t2s_decode_steps ignores the bit, as before: the slot samples
    model.buf["state"].copy_(model._slot_records(ctx, limit=L, flags=2))
    model.buf["x"][:1].copy_(model.start[None, :])
    model._uniform_view(1)[0, :16].fill_(0.5)
    model._run_steps(1.0, 1, 2)
    torch.cuda.synchronize()
    assert model.buf["state"][0].tolist()[0] == 2


# ---------------------------------------------------------------- 5. off = untouched
@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_nothing_moves_when_the_feature_is_off(name):
    from covomix_amd import _lib
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_small(name)
    model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN)
    src, uni, gold_streams = _golden(g)
    flat, streams = model.generate(src, uniforms=uni, return_streams=True)
    assert torch.equal(streams.cpu(), gold_streams[:, :streams.shape[1]])
    if gold_streams.shape[1] == g["streams"].shape[-1]:                       # (the golden decode fits into MAX_LEN steps)
        assert torch.equal(flat.cpu(), torch.from_numpy(g["tokens"]))
    keys = set(model._graphs)
    assert len(keys) == 1 and "logprobs" not in model.buf
    again = model.generate(src, uniforms=uni, return_streams=True, return_logprobs=False)
    assert torch.equal(again[0], flat) and torch.equal(again[1], streams) and len(again) == 2
    assert torch.equal(model.generate(src, uniforms=uni), flat)
    assert set(model._graphs) == keys and "logprobs" not in model.buf
    many = model.generate_many([src, src], [uni, uni], slots=2, return_logprobs=False)
    assert torch.equal(many[0][1], streams.cpu()) and len(many[0]) == 2 and "logprobs" not in model.buf
    keys = set(model._graphs)
    lp = model.generate(src, uniforms=uni, return_logprobs=True)              # on: one more graph, the old ones stay
    assert torch.equal(lp[0], flat) and keys < set(model._graphs) and "logprobs" in model.buf
    assert _lib.load().cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- 6. facade and CLI
@pytest.mark.parametrize("name,cond_scale", [("cosingle_small", 1.0), ("comix_small", 1.0), ("cosingle_small", CFG)])
def test_facade_best_of_and_scoring(name, cond_scale):
    from covomix_amd.conditional_model import CoVoMixModel
    from covomix_amd.t2s import best_candidate, sequence_logprob
    g, sd = load_small(name)
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval().to(DEV)
    S, V, N, steps = g["uniforms"].shape[1], g["uniforms"].shape[-1], 3, 24
    eos = V - 1
    ids = _texts(g, 2, seed=7)
    gen = torch.Generator().manual_seed(5)
    us = [torch.rand(N, steps, S, V, generator=gen).clamp_(1e-6, 1 - 1e-6) for _ in ids]
    kw = dict(cond_scale=cond_scale, max_length=steps)
    for i_, u_ in zip(ids, us):
        cands = [m.synthesis_sample_text2semantic(i_, uniforms=u_[c], return_logprobs=True, best_of=1, **kw) for c in range(N)]
        scores = [sequence_logprob(c[2], c[1], eos) for c in cands]
        best = cands[best_candidate(scores)]
        print(name, cond_scale, "candidate scores", [round(s_, 4) for s_ in scores])
        assert len(set(scores)) == N, "the candidates do not differ"
        assert torch.equal(m.synthesis_sample_text2semantic(i_, uniforms=u_, best_of=N, **kw), best[0])
        full = m.synthesis_sample_text2semantic(i_, uniforms=u_, best_of=N, return_logprobs=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip(full, best)) and len(full) == 3
        # best_of = 1 is the call without it
        today = m.synthesis_sample_text2semantic(i_, uniforms=u_[0], **kw)
        assert torch.equal(m.synthesis_sample_text2semantic(i_, uniforms=u_[0], best_of=1, **kw), today) and torch.equal(today, cands[0][0])
    both = m.synthesis_sample_text2semantic(ids, uniforms=us, best_of=N, slots=4, **kw)
    for j in range(2):
        assert torch.equal(both[j], m.synthesis_sample_text2semantic(ids[j], uniforms=us[j], best_of=N, **kw))
    # scoring: lists == one by one, and == the log-probs sampling returned
    res = [m.synthesis_sample_text2semantic(i_, uniforms=u_[0], return_logprobs=True, **kw) for i_, u_ in zip(ids, us)]
    lst = m.score_text2semantic(ids, [r[1] for r in res], cond_scale=cond_scale)
    for j in range(2):
        single = m.score_text2semantic(ids[j], res[j][1], cond_scale=cond_scale)
        assert torch.equal(single, lst[j]) and torch.equal(single, res[j][2].cpu())
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], uniforms=us[0], best_of=2, **kw)
    if cond_scale == 1.0:
        plain = CoVoMixModel(sd, hparams={"text2semantic": True}).eval().to(DEV)
        with pytest.raises(AssertionError):
            plain.score_text2semantic(ids[0], res[0][1], cond_scale=CFG)


def test_cli_best_of(tmp_path, monkeypatch):
    """a two-turn dialogue: --t2s_best_of 1 writes byte-identical files to a run without the flag; --t2s_best_of 2 runs, decodes two
    candidates per turn and writes the same file names"""
    import covomix_amd.synthetic as syn
    from covomix_amd import generation
    from test_generation_gpu import _write_fixture
    tmp = str(tmp_path)
    _write_fixture(tmp, "vosingle")
    shapes = syn.t2s_param_shapes(two_output=False, dim=64, dim_target=64, source_depth=2, target_depth=2, heads=1, num_text=200)
    tsd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=0).items()}
    torch.save({"state_dict": {"cfm_wrapper.model." + k: v for k, v in tsd.items()},
                "hyper_parameters": {"text2semantic": True}}, os.path.join(tmp, "t2s.ckpt"))
    tdir, pdir = os.path.join(tmp, "text"), os.path.join(tmp, "prompt")
    os.makedirs(tdir); os.makedirs(pdir)
    rng = np.random.RandomState(1)
    for suf in ("_1", "_2"):
        np.save(os.path.join(pdir, f"dlg_a{suf}.hubert_code.npy"), rng.randint(0, 500, size=20))
        np.save(os.path.join(pdir, f"dlg_a{suf}.mel.npy"), (rng.randn(80, 20) * 2 - 6).astype(np.float32))
    for k in range(2):
        np.save(os.path.join(tdir, f"dlg_a.turn{k}.text_ids.npy"), rng.randint(1, 199, size=(1, 7 + k)).astype(np.int64))
    real = generation.CoVoMixModel.synthesis_sample_text2semantic
    seen = []

    def spy(self, ids, **kw):
        seen.append((kw.get("best_of", 1), [tuple(u.shape) for u in kw["uniforms"]]))
        return real(self, ids, max_length=12, **kw)
    monkeypatch.setattr(generation.CoVoMixModel, "synthesis_sample_text2semantic", spy)
    base = ["--t2s_ckpt", os.path.join(tmp, "t2s.ckpt"), "--acous_ckpt", os.path.join(tmp, "acous.ckpt"),
            "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"), "--text_dir", tdir, "--prompt_dir", pdir, "--mode", "covosingle"]
    with pytest.warns(UserWarning, match="EMA"):
        for out, extra in (("o0", []), ("o1", ["--t2s_best_of", "1"]), ("o2", ["--t2s_best_of", "2"])):
            assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, out)] + extra) == 1
    files = [sorted(os.listdir(os.path.join(tmp, o))) for o in ("o0", "o1", "o2")]
    assert files[0] == files[1] == files[2] and "dlg_a.wav" in files[0]
    for f in files[0]:
        if f.endswith(".wav"):
            a, b = (open(os.path.join(tmp, o, f), "rb").read() for o in ("o0", "o1"))
            assert a == b, f
    assert [s_[0] for s_ in seen] == [1, 1, 2]
    assert seen[0][1] == seen[1][1] and all(len(sh) == 3 for sh in seen[0][1])
    assert all(len(sh) == 4 and sh[0] == 2 for sh in seen[2][1]) and len(seen[2][1]) == 2


# ---------------------------------------------------------------- 7. descriptors the scored entry refuses
def test_scored_entry_refuses_bad_descriptors(decoders):
    """CVX_EINVAL and nothing launched: the slot records keep the pattern written before the call"""
    from covomix_amd import _lib, ops
    g, sd, model = decoders["cosingle_small"]
    lib = _lib.load()
    V = model.d["vocab"]
    model._ensure(8, 8, 16, True)
    sentinel = torch.full_like(model.buf["state"], 5)          # position 5 of 40: a launch would advance it
    model.buf["state"].copy_(sentinel)
    lp = model.buf["logprobs"]
    lp.fill_(3.0)
    size = C.sizeof(_lib.T2SScoring)
    assert size == 16

    def call(scoring=None, **edit):
        dec = model._descriptor(1.0, edit.pop("batch", 8), edit.pop("cfg_scale", 1.0), edit.pop("queue", False), None, edit.pop("nd", 0))
        for name, v in edit.items():
            setattr(dec, name, v)
        sc = _lib.T2SScoring(size, MAX_LEN, lp.data_ptr()) if scoring is None else _lib.T2SScoring(*scoring)
        rc = lib.cvx_t2s_decode_steps_scored(C.byref(dec), C.byref(sc), 1, ops._stream())
        torch.cuda.synchronize()
        return rc

    assert call(scoring=(size - 4, MAX_LEN, lp.data_ptr())) == EINVAL       # a short struct
    assert call(scoring=(size + 8, MAX_LEN, lp.data_ptr())) == EINVAL       # a size this library does not know
    assert call(scoring=(0, MAX_LEN, lp.data_ptr())) == EINVAL
    assert call(scoring=(size, MAX_LEN, None)) == EINVAL                    # NULL logprobs
    assert call(scoring=(size, MAX_LEN - 1, lp.data_ptr())) == EINVAL       # rows not laid out like those of tokens
    dec = model._descriptor(1.0, 8)
    assert lib.cvx_t2s_decode_steps_scored(C.byref(dec), None, 1, ops._stream()) == EINVAL
    # the inherited descriptor checks
    assert call(cfg_scale=CFG, queue=True, nd=7) == EINVAL and call(cfg_scale=CFG, queue=True, nd=0) == EINVAL
    assert call(top_k=0) == EINVAL and call(top_k=V + 1) == EINVAL
    assert call(filter_mode=2) == EINVAL and call(filter_mode=1, top_p=1.0) == EINVAL
    assert call(batch=65) == EINVAL and call(vocab=1025) == EINVAL and call(state=None) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(model.buf["state"], sentinel) and bool((lp == 3.0).all())
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION
