"""GPU: text2semantic beam search on the decode slots (cvx_t2s_beam_steps, cvx_t2s_beam_select_f32, TextToSemanticDecoder.generate_beam).

  4. the selection entry against the fp64 restatement on the crafted blocks of tests/t2s_beam_restated.py;
  5. beam_size 1 (identity ancestry) == the greedy decode of the direct kernels, log-probs bit for bit;
  6. every hypothesis' log-probs == its teacher-forced score, its score == their fp32 sum in the selection's association - with re-parenting;
  7. the search against the fp64 oracle beam search over the decidable prefix;
  8. an utterance alone == the same utterance among neighbours (9, 60, 64 slots) and in waves;
  9. finished hypotheses end to end (an adjusted eos embedding row), length_penalty;
 10. nothing moves for the sampling paths; 11. refusals launch nothing; 12. the facade; 13. the CLI flag.
The fixtures are the committed cosingle_small / comix_small models with max_length = 40."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import t2s_beam_restated as br
import t2s_logprob_restated as rs
from test_t2s_filters import decode_uniforms, load_small

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
MAX_LEN = 40
NAMES = ("cosingle_small", "comix_small")


@pytest.fixture(scope="module")
def decoders():
    from covomix_amd.t2s import TextToSemanticDecoder
    out = {}
    for name in NAMES:
        g, sd = load_small(name)
        out[name] = (g, sd, TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN))
    return out


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


def _fp32_score(lp):
    """the selection's accumulation of a hypothesis' log-probs [S, L]: c + lp0, or c + (lp0 + lp1), step by step in fp32"""
    c = torch.zeros((), dtype=torch.float32)
    for t in range(lp.shape[1]):
        c = c + lp[0, t] if lp.shape[0] == 1 else c + (lp[0, t] + lp[1, t])
    return float(c)


def _same(a, b):
    return all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b)) and len(a) == len(b)


def _reparented_steps(rec, slot, steps):
    """steps of the hypothesis in `slot` at which it came from another slot"""
    from covomix_amd.t2s import beam_backtrack
    path = beam_backtrack(rec["parents"], rec["tokens"], rec["logprobs"], slot, steps)[2]
    return sum(1 for t in range(steps) if int(rec["parents"][t, path[t]]) != path[t])


# ---------------------------------------------------------------- 4. the selection entry
@pytest.mark.parametrize("V", br.VOCABS)
def test_select_entry_against_the_restatement(V):
    from covomix_amd import ops
    worst = 0.0
    for B in br.BEAMS:
        for S in (1, 2):
            lg, sc, fin = br.block(B, S, V)
            assert br.decidable(lg, sc, fin, B), (B, S, V)            # before any device result is looked at
            ref = br.select(lg, sc, fin, B, torch.float64)
            par, tok, lp, out, ofin = (t.cpu() for t in ops.t2s_beam_select(lg.to(DEV), sc.to(DEV), fin.to(DEV), B))
            what = (B, S, V)
            assert torch.equal(par, ref["parents"]) and torch.equal(tok, ref["tokens"]) and torch.equal(ofin, ref["finished"]), what
            worst = max(worst, float(rs.ulps(lp, ref["token_lp"]).max()))
            assert bool(((lp.double() - ref["token_lp"]).abs() <= rs.bound(ref["token_lp"])).all()), what
            base = (torch.arange(3 * B) // B) * B
            c = sc[base + par.long()]
            want = torch.where(tok[:, 0] >= 0, c + lp[:, 0] if S == 1 else c + (lp[:, 0] + lp[:, 1]), c)
            want = torch.where(ref["scores"] > -math.inf, want, torch.full_like(want, -math.inf))      # dead slots
            assert torch.equal(out, want), what
            for g_ in range(3):                                         # a group alone == the group among others
                sl = slice(g_ * B, (g_ + 1) * B)
                one = [t.cpu() for t in ops.t2s_beam_select(lg[sl].to(DEV), sc[sl].to(DEV), fin[sl].to(DEV), B)]
                assert all(torch.equal(a, b[sl]) for a, b in zip(one, (par, tok, lp, out, ofin))), (what, g_)
    print(f"V = {V}: largest token log-prob error {worst:.2f} units of 2^-24 (1 + |lp|)")


# ---------------------------------------------------------------- 5. identity ancestry == direct attention
@pytest.mark.parametrize("name", NAMES)
def test_beam_size_one_is_the_greedy_decode(decoders, name):
    g, sd, model = decoders[name]
    src = torch.from_numpy(g["source_ids"])
    S, V = model.d["streams"], model.d["vocab"]
    flat, streams, lp = model.generate(src, uniforms=decode_uniforms(S, V)[:MAX_LEN], filter_logits_fn="top_k", filter_fn_kwargs={"k": 1},
                                       return_logprobs=True)
    bflat, bstreams, blp, score = model.generate_beam(src, beam_size=1)
    assert torch.equal(bflat, flat.cpu()) and torch.equal(bstreams, streams.cpu())
    assert torch.equal(blp, lp.cpu()) and blp.dtype == torch.float32
    assert score == _fp32_score(blp)
    assert bool((model.last_beam[0]["parents"] == 0).all())


# ---------------------------------------------------------------- 6. bit-identity with forced scoring
@pytest.mark.parametrize("name", NAMES)
def test_hypotheses_equal_their_forced_score(decoders, name):
    from covomix_amd.t2s import beam_backtrack
    g, sd, model = decoders[name]
    src = torch.from_numpy(g["source_ids"])
    most = 0
    for B in (2, 3, 4, 10):
        beams = model.generate_beam(src, beam_size=B, return_beams=True)
        rec = model.last_beam[0]
        assert len(beams) == B and rec["steps"] == MAX_LEN
        scored = model.score_many([src] * B, [h[1] for h in beams])
        for i, (flat, streams, lp, score) in enumerate(beams):
            slot = rec["order"][i]
            assert streams.shape == (model.d["streams"], MAX_LEN) and lp.dtype == torch.float32
            assert torch.equal(lp, scored[i]), (name, B, i)
            assert score == _fp32_score(lp) == float(rec["scores"][slot]), (name, B, i)
            tk, hl, _ = beam_backtrack(rec["parents"], rec["tokens"], rec["logprobs"], slot, MAX_LEN)      # the device's back-track
            assert torch.equal(tk.long(), streams) and torch.equal(hl, lp), (name, B, i)
            most = max(most, _reparented_steps(rec, slot, MAX_LEN))
        vals = [h[3] / (MAX_LEN * model.d["streams"]) for h in beams]
        assert vals == sorted(vals, reverse=True) and _same(beams[0], model.generate_beam(src, beam_size=B))
    print(f"{name}: a returned hypothesis changed slots at {most} steps")
    assert most >= 4, "no returned hypothesis was re-parented at four or more steps: the ancestry table was not exercised"


# ---------------------------------------------------------------- 7. against the fp64 oracle
ORACLE_CASES = [("cosingle_small", 12, 3), ("cosingle_small", 12, 4), ("comix_small", 9, 2)]


@pytest.mark.parametrize("name,ids,B", ORACLE_CASES)
def test_against_the_oracle_beam_search(decoders, name, ids, B):
    """Measured with the fp64 oracle on the CPU, the bound holding both terms: decidable prefixes of 19, 19 and 18 steps with 14, 16 and
    17 re-parenting steps (the full 12-id text on comix_small at B = 2 reaches 5 steps only and is not used)."""
    g, sd, model = decoders[name]
    src = torch.from_numpy(g["source_ids"])[:, :ids]
    steps = br.oracle_beam(sd, src, B, MAX_LEN)
    n, acc = br.decidable_prefix(steps)
    moved = sum(1 for s in steps[:n] if any(h[3] != i for i, h in enumerate(s["hyps"])))
    print(f"{name}, {ids} ids, B = {B}: decidable prefix {n} steps, {moved} of them re-parent, accumulated bound {acc[n - 1]:.3e}")
    assert n >= 12 and moved >= 4, "the oracle alone does not meet the conditions of this check"
    model.generate_beam(src, beam_size=B)
    got = br.replay(*(model.last_beam[0][k] for k in ("parents", "tokens", "logprobs")))
    worst = 0.0
    for t in range(n):
        want = {h[0]: h[1] for h in steps[t]["hyps"]}
        have = {pre: float(c) for pre, c in got[t]}
        assert set(have) == set(want), (name, B, t)
        for pre in want:
            worst = max(worst, abs(have[pre] - want[pre]) / acc[t])
            assert abs(have[pre] - want[pre]) <= acc[t], (name, B, t)
    print(f"largest score error / accumulated bound {worst:.3f}")


# ---------------------------------------------------------------- 8. slots, neighbours, gemv groups, waves
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("B,n,check", [(3, 3, (1, 2)), (10, 6, (0, 5)), (16, 5, (0, 1, 2, 3, 4))])
def test_an_utterance_does_not_depend_on_its_neighbours(decoders, name, B, n, check):
    """B = 3: 9 slots, the second utterance in slots 3-5, the third across the 8-slot group boundary; B = 10: 60 slots; B = 16: five
    utterances = a wave of four (64 slots) and a wave of one"""
    g, sd, model = decoders[name]
    srcs = _texts(g, n, seed=40 + B)
    assert len({s_.shape[1] for s_ in srcs}) > 1
    wave = model.generate_beam(srcs, beam_size=B, return_beams=True)
    recs = model.last_beam
    assert len(wave) == n and len(recs) == n
    for j in check:
        alone = model.generate_beam(srcs[j], beam_size=B, return_beams=True)
        assert all(_same(a, b) for a, b in zip(alone, wave[j])) and len(alone) == B, (name, B, j)
        assert torch.equal(model.last_beam[0]["parents"], recs[j]["parents"])


# ---------------------------------------------------------------- 9. finished hypotheses
@pytest.mark.parametrize("name,tok,alpha,B", [("cosingle_small", 95, 1.2, 3), ("comix_small", 400, 1.01, 3)])
def test_finished_hypotheses_end_to_end(name, tok, alpha, B):
    """the eos embedding row = alpha * the row of a token the greedy decode repeats (the logits are tied to the embedding): measured with the
    fp64 oracle, the hypotheses finish at steps 0, 3, 4 (cosingle_small; the search ends after 5 steps, all of them decidable) and
    0, 1, 2 (comix_small, 3 steps)"""
    from covomix_amd.t2s import TextToSemanticDecoder, beam_rank
    g, sd = load_small(name)
    sd = dict(sd)
    E = sd["semantic_token_emb.weight"].clone()
    E[-1] = alpha * E[tok]
    sd["semantic_token_emb.weight"] = E
    src = torch.from_numpy(g["source_ids"])
    eos = E.shape[0] - 1
    steps = br.oracle_beam(sd, src, B, MAX_LEN)
    first = {}
    for t, s in enumerate(steps):
        for h in s["hyps"]:
            if h[2] and h[1] > -math.inf:
                first.setdefault(h[0], t)
    assert steps[-1]["ended"] and len(steps) < MAX_LEN and len(set(first.values())) > 1, "the oracle search does not end early"
    n, acc = br.decidable_prefix(steps)
    model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN)
    beams = model.generate_beam(src, beam_size=B, return_beams=True, length_penalty=1.0)
    rec = model.last_beam[0]
    T = rec["steps"]
    print(f"{name}: oracle ends after {len(steps)} steps (finishing at {sorted(first.values())}, decidable prefix {n}); device after {T}, "
          f"lengths {rec['lengths']}")
    assert T < MAX_LEN, "the search did not end early"
    if n == len(steps):                                               # every step decidable: the same search
        assert T == len(steps)
        got = br.replay(rec["parents"], rec["tokens"], rec["logprobs"])
        assert {pre for pre, _ in got[-1]} == {h[0] for h in steps[-1]["hyps"]}
    assert len(set(rec["lengths"])) > 1, "the hypotheses finished at the same step"
    S = model.d["streams"]
    scored = model.score_many([src] * B, [h[1] for h in beams])
    for i, (flat, streams, lp, score) in enumerate(beams):
        slot = rec["order"][i]
        L = rec["lengths"][slot]
        assert streams.shape == (S, L) and bool((streams[:, L - 1] == eos).any()) and not bool((streams[:, :L - 1] == eos).any())
        assert torch.equal(lp, scored[i]) and score == _fp32_score(lp) == float(rec["scores"][slot]), (name, i)
        # carried from its eos step on: the records of the later steps name the hypothesis itself and nothing new
        path = br.replay(rec["parents"], rec["tokens"], rec["logprobs"])
        assert float(path[T - 1][slot][1]) == score and len(path[T - 1][slot][0]) == L
    for pen in (0.0, 1.0):
        want = max(range(B), key=lambda i: (float(rec["scores"][i]) / (rec["lengths"][i] * S) ** pen, -i))
        assert beam_rank(rec["scores"], rec["lengths"], S, pen)[0] == want
        best = model.generate_beam(src, beam_size=B, length_penalty=pen)
        assert torch.equal(model.last_beam[0]["parents"], rec["parents"])
        assert best[3] == float(rec["scores"][want]) and best[1].shape[1] == rec["lengths"][want], (name, pen)


# ---------------------------------------------------------------- 10. unused = untouched
@pytest.mark.parametrize("name", NAMES)
def test_nothing_moves_for_the_sampling_paths(name):
    from covomix_amd import _lib
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_small(name)
    model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN)
    src = torch.from_numpy(g["source_ids"])
    S, V = model.d["streams"], model.d["vocab"]
    uni = decode_uniforms(S, V)[:MAX_LEN]

    def run():
        one = model.generate(src, uniforms=uni, return_logprobs=True)
        many = model.generate_many([src, src[:, :7]], [uni, uni], slots=2)
        return [t.cpu() for t in one] + [t for r in many for t in r] + model.score_many([src], [one[1]])
    before = run()
    keys = set(model._graphs)
    assert getattr(model, "_beam", None) is None and len(keys) == 3
    model.generate_beam(src, beam_size=4)
    added = set(model._graphs) - keys
    assert keys <= set(model._graphs) and len(added) == 1 and all(k[0] == "beam" and k[1] == 4 for k in added)
    after = run()
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and len(before) == len(after)
    assert set(model._graphs) == keys | added
    assert _lib.load().cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- 11. refusals launch nothing
def test_beam_entries_refuse_and_launch_nothing(decoders):
    from covomix_amd import _lib, ops
    g, sd, model = decoders["cosingle_small"]
    lib = _lib.load()
    model._ensure(8, 8, 0)
    bm = model._ensure_beam()
    sentinel = torch.full_like(model.buf["state"], 5)                  # position 5 of 40: a launch would advance it
    model.buf["state"].copy_(sentinel)
    groups = torch.tensor([[5, 0, MAX_LEN, 0]] * bm["groups"].shape[0], dtype=torch.int32, device=DEV)
    bm["groups"].copy_(groups)
    bm["scores"].fill_(-3.0)
    bm["logprobs"].fill_(7.0)
    names = ("scores", "finished", "owner", "groups", "parents", "hist_tokens", "hist_logprobs", "short_lp", "short_tokens", "logprobs")
    size = C.sizeof(_lib.T2SBeam)
    assert size == 16 + 8 * len(names)

    def call(beam=True, struct_size=size, beam_size=2, hist_len=MAX_LEN, backtrack=1, null=None, **edit):
        dec = model._descriptor(1.0, edit.pop("batch", 8), edit.pop("cfg_scale", 1.0), edit.pop("queue", False), None, edit.pop("nd", 0))
        for name, v in edit.items():
            setattr(dec, name, v)
        bs = _lib.T2SBeam(struct_size, beam_size, hist_len, backtrack, *[None if k == null else bm[k].data_ptr() for k in names])
        rc = lib.cvx_t2s_beam_steps(C.byref(dec), C.byref(bs) if beam else None, 1, ops._stream())
        torch.cuda.synchronize()
        return rc

    assert call(beam=False) == EINVAL
    assert call(struct_size=size - 8) == EINVAL and call(struct_size=size + 8) == EINVAL and call(struct_size=0) == EINVAL
    assert call(queue=True, nd=8) == EINVAL                             # a dialogue queue
    assert call(cfg_scale=1.5) == EINVAL                                # guidance
    for b_ in (0, -1, 17, 3, 5):                                        # outside [1, 16], or no divisor of batch = 8
        assert call(beam_size=b_) == EINVAL, b_
    assert call(beam_size=16, batch=8) == EINVAL
    assert call(hist_len=MAX_LEN - 1) == EINVAL
    for k in names:
        assert call(null=k) == EINVAL, k
    assert call(batch=65) == EINVAL and call(vocab=1025) == EINVAL and call(state=None) == EINVAL      # the inherited descriptor checks
    assert torch.equal(model.buf["state"], sentinel) and torch.equal(bm["groups"], groups)
    assert bool((bm["scores"] == -3.0).all()) and bool((bm["logprobs"] == 7.0).all())
    # the selection entry
    B, S, V = 2, 2, 16
    lg = torch.zeros(2 * B, S, V, device=DEV)
    sc = torch.zeros(2 * B, device=DEV)
    fin = torch.zeros(2 * B, dtype=torch.uint8, device=DEV)
    outs = [torch.full((2 * B,), 9, dtype=torch.int32, device=DEV), torch.full((2 * B, S), 9, dtype=torch.int64, device=DEV),
            torch.full((2 * B, S), 9.0, device=DEV), torch.full((2 * B,), 9.0, device=DEV), torch.full((2 * B,), 9, dtype=torch.uint8, device=DEV)]

    def sel(groups=2, beam_size=B, streams=S, vocab=V, null=None):
        ptr = [None if null == i else t.data_ptr() for i, t in enumerate([lg, sc, fin] + outs)]
        rc = lib.cvx_t2s_beam_select_f32(ptr[0], ptr[1], ptr[2], groups, beam_size, streams, vocab, *ptr[3:], ops._stream())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(beam_size=0), dict(beam_size=17), dict(streams=0), dict(streams=3), dict(vocab=0), dict(vocab=1025), dict(groups=-1)):
        assert sel(**kw) == EINVAL, kw
    for i in range(8):
        assert sel(null=i) == EINVAL, i
    assert sel(groups=0) == 0                                           # no groups: nothing to do
    assert all(bool((t == 9).all()) for t in outs)
    assert sel() == 0 and outs[0].tolist() == [0, 0, 0, 0] and outs[1][:, 0].tolist() == [0, 0, 0, 0] and outs[1][:, 1].tolist() == [0, 1, 0, 1]
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- 12. the facade
@pytest.mark.parametrize("name", NAMES)
def test_facade_beam_search(decoders, name):
    from covomix_amd.conditional_model import CoVoMixModel
    g, sd, model = decoders[name]
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval().to(DEV)
    ids = _texts(g, 3, seed=9)
    kw = dict(beam_search_decode=True, beam_size=4, max_length=24)
    want = [model.generate_beam(i_, beam_size=4, max_length=24) for i_ in ids]
    flat = m.synthesis_sample_text2semantic(ids[0].to(DEV), **kw)
    assert flat.device.type == "cuda" and torch.equal(flat.cpu(), want[0][0])
    full = m.synthesis_sample_text2semantic(ids[0], return_logprobs=True, **kw)
    assert len(full) == 3 and all(torch.equal(a, b) for a, b in zip(full, want[0][:3]))
    lst = m.synthesis_sample_text2semantic(ids, **kw)
    assert len(lst) == 3 and all(torch.equal(a, w[0]) for a, w in zip(lst, want))
    lst = m.synthesis_sample_text2semantic(ids, return_logprobs=True, **kw)
    assert all(torch.equal(a[2], w[2]) for a, w in zip(lst, want))
    ten = m.synthesis_sample_text2semantic(ids[0], beam_search_decode=True, max_length=24)                 # the reference's default: 10
    assert torch.equal(ten, model.generate_beam(ids[0], beam_size=10, max_length=24)[0])
    pen = m.synthesis_sample_text2semantic(ids[0], length_penalty=0.0, return_logprobs=True, **kw)
    assert torch.equal(pen[1], model.generate_beam(ids[0], beam_size=4, max_length=24, length_penalty=0.0)[1])
    # sampling controls play no part
    assert torch.equal(m.synthesis_sample_text2semantic(ids[0], temprature=0.3, filter_logits_fn="top_p", **kw), want[0][0])
    S, V = model.d["streams"], model.d["vocab"]
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], uniforms=torch.rand(24, S, V), **kw)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], generator=torch.Generator(device=DEV), **kw)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], best_of=2, **kw)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], beam_search_decode=True, beam_size=17)
    with pytest.raises(NotImplementedError, match="guidance"):
        m.synthesis_sample_text2semantic(ids[0], cond_scale=1.5, **kw)


# ---------------------------------------------------------------- 13. the CLI flag
def test_cli_beam_size(tmp_path, monkeypatch):
    """a two-turn dialogue: --t2s_beam_size 0 writes byte-identical files to a run without the flag; --t2s_beam_size 4 runs beam search per
    turn (no draws) and writes the same file names"""
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
        seen.append((kw.get("beam_search_decode", False), kw.get("beam_size"), "uniforms" in kw, len(ids)))
        return real(self, ids, max_length=12, **kw)
    monkeypatch.setattr(generation.CoVoMixModel, "synthesis_sample_text2semantic", spy)
    base = ["--t2s_ckpt", os.path.join(tmp, "t2s.ckpt"), "--acous_ckpt", os.path.join(tmp, "acous.ckpt"),
            "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"), "--text_dir", tdir, "--prompt_dir", pdir, "--mode", "covosingle"]
    with pytest.warns(UserWarning, match="EMA"):
        for out, extra in (("o0", []), ("o1", ["--t2s_beam_size", "0"]), ("o2", ["--t2s_beam_size", "4"])):
            assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, out)] + extra) == 1
    files = [sorted(os.listdir(os.path.join(tmp, o))) for o in ("o0", "o1", "o2")]
    assert files[0] == files[1] == files[2] and "dlg_a.wav" in files[0]
    for f in files[0]:
        if f.endswith(".wav"):
            a, b = (open(os.path.join(tmp, o, f), "rb").read() for o in ("o0", "o1"))
            assert a == b, f
    assert seen == [(False, None, True, 2), (False, None, True, 2), (True, 4, False, 2)]
    with pytest.raises(ValueError, match="t2s_beam_size"):
        generation.run(True, base + ["--saved_dir", os.path.join(tmp, "o3"), "--t2s_beam_size", "4", "--t2s_best_of", "2"])
