"""GPU: text2semantic beam search under classifier-free guidance (cvx_t2s_beam_guided_steps, cvx_t2s_beam_guided_queue_steps,
TextToSemanticDecoder.generate_beam / generate_beam_many with cond_scale > 1): a hypothesis is a slot pair with one ancestry.

  6. beam_size 1 (identity ancestry of both halves) == the guided greedy decode of the direct kernels, bit for bit;
  7. every hypothesis' log-probs == score_many(cond_scale=s), its score == their fp32 sum, the device back-track == beam_backtrack - with
     re-parenting;
  8. the search against the fp64 oracle search over the decidable prefix (tests/t2s_beam_guided_restated.py);
  9. finished hypotheses end to end, length_penalty;
 10. an utterance alone == the same utterance among neighbours and in waves;
 11. the queue form == generate_beam alone;
 12. nothing moves for the other paths; 13. refusals launch nothing; 14. the facade switch; 15. the CLI flag.
The fixture is the committed cosingle_small model with max_length = 40 (guidance runs on one-output models)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import t2s_beam_guided_restated as bg
import t2s_beam_restated as br
from test_t2s_filters import decode_uniforms, load_small

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
MAX_LEN = bg.MAX_LEN
NAME = "cosingle_small"


@pytest.fixture(scope="module")
def decoder():
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_small(NAME)
    return g, sd, TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN)


def _texts(g, n, seed):
    """n texts of different length cut from the golden one (the first is the golden text itself)"""
    src = torch.from_numpy(g["source_ids"])
    gen = torch.Generator().manual_seed(seed)
    L = src.shape[1]
    out = [src]
    for i in range(1, n):
        a = int(torch.randint(0, max(1, L // 2), (1,), generator=gen))
        e = int(torch.randint(a + 3, L + 1, (1,), generator=gen))
        out.append(src[:, a:e] if i % 5 else torch.cat((src, src[:, : 1 + i % 7]), dim=1))
    return out


def _fp32_score(lp):
    """the selection's accumulation of a hypothesis' log-probs [1, L]: c + lp, step by step in fp32"""
    c = torch.zeros((), dtype=torch.float32)
    for t in range(lp.shape[1]):
        c = c + lp[0, t]
    return float(c)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


def _same_record(a, b, keys=("parents", "tokens", "logprobs", "lengths", "order", "steps")):
    return all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in keys) and torch.equal(a["scores"], b["scores"])


def _reparented_steps(rec, slot, steps):
    """steps of the hypothesis in `slot` at which it came from another slot"""
    from covomix_amd.t2s import beam_backtrack
    path = beam_backtrack(rec["parents"], rec["tokens"], rec["logprobs"], slot, steps)[2]
    return sum(1 for t in range(steps) if int(rec["parents"][t, path[t]]) != path[t])


# ---------------------------------------------------------------- 6. identity ancestry of both halves == the direct kernels
@pytest.mark.parametrize("scale", [1.5, 3.0])
def test_beam_size_one_is_the_guided_greedy_decode(decoder, scale):
    g, sd, model = decoder
    src = torch.from_numpy(g["source_ids"])
    V = model.d["vocab"]
    flat, streams, lp = model.generate(src, uniforms=decode_uniforms(1, V)[:MAX_LEN], filter_logits_fn="top_k", filter_fn_kwargs={"k": 1},
                                       return_logprobs=True, cond_scale=scale)
    bflat, bstreams, blp, score = model.generate_beam(src, beam_size=1, cond_scale=scale)
    assert torch.equal(bflat, flat.cpu()) and torch.equal(bstreams, streams.cpu())
    assert torch.equal(blp, lp.cpu()) and blp.dtype == torch.float32
    assert score == _fp32_score(blp)
    assert bool((model.last_beam[0]["parents"] == 0).all())


# ---------------------------------------------------------------- 7. bit-identity with guided forced scoring
@pytest.mark.parametrize("scale", [1.5, 3.0])
def test_hypotheses_equal_their_guided_forced_score(decoder, scale):
    from covomix_amd.t2s import beam_backtrack
    g, sd, model = decoder
    src = torch.from_numpy(g["source_ids"])
    most = 0
    for B in (2, 3, 4, 10, 16):
        beams = model.generate_beam(src, beam_size=B, return_beams=True, cond_scale=scale)
        rec = model.last_beam[0]
        assert len(beams) == B and rec["steps"] == MAX_LEN and rec["parents"].shape == (MAX_LEN, B)
        scored = model.score_many([src] * B, [h[1] for h in beams], cond_scale=scale)
        for i, (flat, streams, lp, score) in enumerate(beams):
            slot = rec["order"][i]
            assert streams.shape == (1, MAX_LEN) and lp.dtype == torch.float32
            assert torch.equal(lp, scored[i]), (scale, B, i)
            assert score == _fp32_score(lp) == float(rec["scores"][slot]), (scale, B, i)
            tk, hl, _ = beam_backtrack(rec["parents"], rec["tokens"], rec["logprobs"], slot, MAX_LEN)      # the device's back-track
            assert torch.equal(tk.long(), streams) and torch.equal(hl, lp), (scale, B, i)
            most = max(most, _reparented_steps(rec, slot, MAX_LEN))
        vals = [h[3] / MAX_LEN for h in beams]
        assert vals == sorted(vals, reverse=True) and _same(beams[0], model.generate_beam(src, beam_size=B, cond_scale=scale))
    print(f"scale {scale}: a returned hypothesis changed slots at {most} steps")
    assert most >= 4, "no returned hypothesis was re-parented at four or more steps: the ancestry of the pairs was not exercised"


# ---------------------------------------------------------------- 8. against the fp64 oracle
@pytest.mark.parametrize("ids,B,scale", bg.ORACLE_CASES)
def test_against_the_guided_oracle_beam_search(decoder, ids, B, scale):
    """Measured with the fp64 oracle on the CPU (tests/test_t2s_beam_guided.py asserts it there): decidable prefixes of 14, 14 and 40 steps
    with 6, 8 and 33 re-parenting steps; the guided and the unguided oracle search differ from step 0 on in all three."""
    g, sd, model = decoder
    full = torch.from_numpy(g["source_ids"])
    src = full[:, :ids]
    steps, n, acc, moved = bg.oracle_case(sd, full, ids, B, scale)
    print(f"{ids} ids, B = {B}, scale {scale}: decidable prefix {n} steps, {moved} of them re-parent, accumulated bound {acc[n - 1]:.3e}")
    assert n >= 12 and moved >= 4, "the oracle alone does not meet the conditions of this check"
    plain = br.oracle_beam(sd, src, B, n)
    differ = [t for t in range(n) if {h[0] for h in steps[t]["hyps"]} != {h[0] for h in plain[t]["hyps"]}]
    print(f"the guided and the unguided oracle search hold different prefixes at {len(differ)} of the {n} steps")
    assert differ, "guidance changes nothing inside the decidable prefix: the check would not see it act"
    model.generate_beam(src, beam_size=B, cond_scale=scale)
    got = br.replay(*(model.last_beam[0][k] for k in ("parents", "tokens", "logprobs")))
    worst = 0.0
    for t in range(n):
        want = {h[0]: h[1] for h in steps[t]["hyps"]}
        have = {pre: float(c) for pre, c in got[t]}
        assert set(have) == set(want), (ids, B, scale, t)
        for pre in want:
            worst = max(worst, abs(have[pre] - want[pre]) / acc[t])
            assert abs(have[pre] - want[pre]) <= acc[t], (ids, B, scale, t)
    print(f"largest score error / accumulated bound {worst:.3f}")


# ---------------------------------------------------------------- 9. finished hypotheses
@pytest.mark.parametrize("alpha,B,scale", bg.FINISHED_CASES)
def test_finished_hypotheses_end_to_end(alpha, B, scale):
    """the eos embedding row = alpha * row 127, the token the guided greedy decode repeats.  Measured with the fp64 oracle: alpha 1.05 -
    the search ends after 3 steps, hypotheses finishing at steps 0, 1, 2; alpha 0.95 - three hypotheses finish at steps 0, 1, 2 and are
    carried beside a live one to the step limit; every step decidable in both."""
    from covomix_amd.t2s import TextToSemanticDecoder, beam_rank
    g, sd = load_small(NAME)
    sd = bg.with_eos_row(sd, alpha)
    src = torch.from_numpy(g["source_ids"])
    eos = sd["semantic_token_emb.weight"].shape[0] - 1
    steps = bg.oracle_beam_guided(sd, src, B, MAX_LEN, scale)
    first = bg.first_finish(steps)
    n, acc = br.decidable_prefix(steps)
    assert n == len(steps) and sorted(first.values())[:3] == [0, 1, 2], "the oracle search is not the one this check was written for"
    assert (steps[-1]["ended"] and len(steps) == 3) if alpha > 1 else (not steps[-1]["ended"] and len(steps) == MAX_LEN)
    model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN)
    beams = model.generate_beam(src, beam_size=B, return_beams=True, length_penalty=1.0, cond_scale=scale)
    rec = model.last_beam[0]
    T = rec["steps"]
    print(f"alpha {alpha}: oracle runs {len(steps)} steps (finishing at {sorted(first.values())}); device {T}, lengths {rec['lengths']}")
    assert T == len(steps)                                            # every step decidable: the same search
    got = br.replay(rec["parents"], rec["tokens"], rec["logprobs"])
    assert {pre for pre, _ in got[-1]} == {h[0] for h in steps[-1]["hyps"]}
    assert len(set(rec["lengths"])) > 1, "the hypotheses finished at the same step"
    scored = model.score_many([src] * B, [h[1] for h in beams], cond_scale=scale)
    n_fin = 0
    for i, (flat, streams, lp, score) in enumerate(beams):
        slot = rec["order"][i]
        L = rec["lengths"][slot]
        assert streams.shape == (1, L)
        if bool((streams == eos).any()):                              # a finished hypothesis: its eos is its last token
            n_fin += 1
            assert bool((streams[:, L - 1] == eos).all()) and not bool((streams[:, :L - 1] == eos).any())
        else:
            assert L == T
        assert torch.equal(lp, scored[i]) and score == _fp32_score(lp) == float(rec["scores"][slot]), (alpha, i)
        # carried from its eos step on: the records of the later steps name the hypothesis itself and nothing new
        assert float(got[T - 1][slot][1]) == score and len(got[T - 1][slot][0]) == L
    assert n_fin == 3
    for pen in (0.0, 1.0):
        want = max(range(B), key=lambda i: (float(rec["scores"][i]) / rec["lengths"][i] ** pen, -i))
        assert beam_rank(rec["scores"], rec["lengths"], 1, pen)[0] == want
        best = model.generate_beam(src, beam_size=B, length_penalty=pen, cond_scale=scale)
        assert torch.equal(model.last_beam[0]["parents"], rec["parents"])
        assert best[3] == float(rec["scores"][want]) and best[1].shape[1] == rec["lengths"][want], (alpha, pen)


# ---------------------------------------------------------------- 10. slots, neighbours, gemv groups, waves
@pytest.mark.parametrize("B,n", [(3, 3), (10, 4), (16, 3)])
def test_an_utterance_does_not_depend_on_its_neighbours(decoder, B, n):
    """B = 3: 18 slots, pairs across the 8-slot gemv groups; B = 10: four utterances = a wave of three (60 slots) and a wave of one;
    B = 16: three utterances = a wave of two (64 slots) and a wave of one"""
    g, sd, model = decoder
    srcs = _texts(g, n, seed=70 + B)
    assert len({s_.shape[1] for s_ in srcs}) > 1
    wave = model.generate_beam(srcs, beam_size=B, return_beams=True, cond_scale=1.5)
    recs = model.last_beam
    assert len(wave) == n and len(recs) == n
    for j in range(n):
        alone = model.generate_beam(srcs[j], beam_size=B, return_beams=True, cond_scale=1.5)
        assert all(_same(a, b) for a, b in zip(alone, wave[j])) and len(alone) == B, (B, j)
        assert torch.equal(model.last_beam[0]["parents"], recs[j]["parents"]) and _same_record(model.last_beam[0], recs[j]), (B, j)


# ---------------------------------------------------------------- 11. the queue form
LIMITS = (5, 40, 17, 16, 33, 7, 24)            # odd / even ends, 16 = a CHUNK boundary


@pytest.mark.parametrize("B,slots", [(3, 18), (10, 64)])
def test_refilled_groups_equal_alone(decoder, B, slots):
    g, sd, model = decoder
    texts = _texts(g, 7, seed=21)
    out = model.generate_beam_many(texts, B, return_beams=True, slots=slots, limits=LIMITS, cond_scale=1.5)
    recs = list(model.last_beam)
    assert len(out) == len(recs) == 7
    G = slots // (2 * B)
    groups = [r["group"] for r in recs]
    print(f"B = {B}: utterance -> group {groups}")
    assert G == 3 and all(0 <= x < G for x in groups) and groups[:G] == list(range(G))
    assert max(groups.count(x) for x in set(groups)) >= 2, "no group decoded two utterances: nothing was refilled"
    for j, (src, lim) in enumerate(zip(texts, LIMITS)):
        alone = model.generate_beam(src, B, max_length=lim, return_beams=True, cond_scale=1.5)
        assert len(out[j]) == B and all(_same(a, b) for a, b in zip(out[j], alone)), (B, j)
        assert _same_record(recs[j], model.last_beam[0]), (B, j)
        assert recs[j]["status"] in (2, 3) and recs[j]["steps"] <= lim and (recs[j]["status"] == 2 or recs[j]["steps"] == lim), (B, j)
    best = model.generate_beam_many(texts, B, slots=slots, limits=LIMITS, cond_scale=1.5)
    assert all(_same(a, h[0]) for a, h in zip(best, out))
    with pytest.raises(ValueError, match="slots"):
        model.generate_beam_many(texts, B, slots=2 * B - 1, cond_scale=1.5)
    with pytest.raises(ValueError, match="cond_scale"):
        model.generate_beam_many(texts, B, cond_scale=0.5)


# ---------------------------------------------------------------- 12. unused = untouched
def test_nothing_moves_for_the_other_paths():
    from covomix_amd import _lib
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_small(NAME)
    model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN)
    src = torch.from_numpy(g["source_ids"])
    V = model.d["vocab"]
    uni = decode_uniforms(1, V)[:MAX_LEN]

    def run():
        one = model.generate(src, uniforms=uni, return_logprobs=True)
        many = model.generate_many([src, src[:, :7]], [uni, uni], slots=2)
        beams = model.generate_beam(src, 4, return_beams=True)
        return [t.cpu() for t in one] + [t for r in many for t in r] + model.score_many([src], [one[1]]) + \
            [t for h in beams for t in h[:3]] + [torch.tensor([h[3] for h in beams])]
    before = run()
    keys = set(model._graphs)
    assert len(keys) == 4
    guided = model.generate_beam(src, beam_size=4, cond_scale=1.5)
    added = set(model._graphs) - keys
    assert keys <= set(model._graphs) and len(added) == 1
    assert all(k[0] == "beamg" and k[1] == 4 and k[2] == 8 and k[3] == 1.5 for k in added)      # its own kind, 4 pairs = 8 slots, the scale
    res = model.generate_beam_many([src, src[:, :7], src[:, :5]], 4, slots=8, cond_scale=1.5)
    added = set(model._graphs) - keys
    assert len(res) == 3 and sorted(k[0] for k in added) == ["beamg", "beamqg"]
    after = run()
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and len(before) == len(after)
    assert set(model._graphs) == keys | added
    # scale 1 is the unguided call: the same key, the same bits
    a = model.generate_beam(src, beam_size=4, return_beams=True)
    b = model.generate_beam(src, beam_size=4, return_beams=True, cond_scale=1.0)
    assert all(_same(x, y) for x, y in zip(a, b)) and set(model._graphs) == keys | added
    assert not _same(a[0], guided)                                    # (and guidance does change the result)
    with pytest.raises(ValueError, match="cond_scale"):
        model.generate_beam(src, beam_size=4, cond_scale=0.5)
    assert _lib.load().cvx_version() == 113 == _lib.ABI_VERSION


def test_two_output_models_are_refused():
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_small("comix_small")
    model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN)
    src = torch.from_numpy(g["source_ids"])
    with pytest.raises(NotImplementedError, match="two-output"):
        model.generate_beam(src, beam_size=2, cond_scale=1.5)
    with pytest.raises(NotImplementedError, match="two-output"):
        model.generate_beam_many([src], 2, cond_scale=1.5)


# ---------------------------------------------------------------- 13. refusals launch nothing
def test_guided_entries_refuse_and_launch_nothing(decoder):
    from covomix_amd import _lib, ops
    g, sd, model = decoder
    lib = _lib.load()
    model._ensure(8, 8, 0)
    bm = model._ensure_beam()
    bq = model._ensure_beam_queue(8)
    sentinel = torch.full_like(model.buf["state"], 5)                  # position 5 of 40: a launch would advance it
    model.buf["state"].copy_(sentinel)
    groups = torch.tensor([[5, 0, MAX_LEN, 0]] * bm["groups"].shape[0], dtype=torch.int32, device=DEV)
    bm["groups"].copy_(groups)
    utter = torch.full_like(bq["utterances"], 3)
    bq["utterances"].copy_(utter)
    queue = torch.tensor([4, 8], dtype=torch.int32, device=DEV)
    bq["queue"].copy_(queue)
    bm["scores"].fill_(-3.0)
    bm["logprobs"].fill_(7.0)
    bq["logprobs"].fill_(7.0)
    bq["final_scores"].fill_(9.0)
    names = ("scores", "finished", "owner", "groups", "parents", "hist_tokens", "hist_logprobs", "short_lp", "short_tokens", "logprobs")
    qnames = ("queue", "utterances", "start", "parents", "hist_tokens", "hist_logprobs", "final_scores", "final_steps", "final_finished",
              "tokens", "logprobs")
    size, qsize = C.sizeof(_lib.T2SBeam), C.sizeof(_lib.T2SBeamQueue)

    def call(entry, beam=True, bqueue=True, struct_size=size, qstruct_size=qsize, beam_size=2, hist_len=MAX_LEN, backtrack=1, null=None,
             qnull=None, n_utterances=8, **edit):
        dec = model._descriptor(1.0, edit.pop("batch", 8), edit.pop("cfg_scale", 1.5), edit.pop("queue", False), None, edit.pop("nd", 0))
        for name, v in edit.items():
            setattr(dec, name, v)
        qform = entry.endswith("queue_steps")
        bs = _lib.T2SBeam(struct_size, beam_size, hist_len, backtrack,
                          *[None if k == null else (bq["owner"] if k == "owner" and qform else bm[k]).data_ptr() for k in names])
        if qform:
            qs = _lib.T2SBeamQueue(qstruct_size, n_utterances,
                                   *[None if k == qnull else (model.start if k == "start" else bq[k]).data_ptr() for k in qnames])
            rc = getattr(lib, entry)(C.byref(dec), C.byref(bs) if beam else None, C.byref(qs) if bqueue else None, 1, ops._stream())
        else:
            rc = getattr(lib, entry)(C.byref(dec), C.byref(bs) if beam else None, 1, ops._stream())
        torch.cuda.synchronize()
        return rc

    for entry in ("cvx_t2s_beam_guided_steps", "cvx_t2s_beam_guided_queue_steps"):
        assert call(entry, beam=False) == EINVAL
        assert call(entry, struct_size=size - 8) == EINVAL and call(entry, struct_size=size + 8) == EINVAL and call(entry, struct_size=0) == EINVAL
        for scale in (1.0, 0.5, 0.0, -2.0, float("nan")):               # not > 1: the unguided entry is the one to call
            assert call(entry, cfg_scale=scale) == EINVAL, scale
        assert call(entry, streams=2) == EINVAL and call(entry, n_ctx=3) == EINVAL
        assert call(entry, queue=True, nd=8) == EINVAL                  # the dialogue queue of the sampled decode
        for b_ in (0, -1, 17, 3, 8, 16):                                # outside [1, 16], or 2 * beam_size no divisor of batch = 8
            assert call(entry, beam_size=b_) == EINVAL, b_
        assert call(entry, beam_size=2, batch=6) == EINVAL and call(entry, beam_size=1, batch=7) == EINVAL
        assert call(entry, hist_len=MAX_LEN - 1) == EINVAL
        for k in names:
            assert call(entry, null=k) == EINVAL, k
        assert call(entry, batch=66) == EINVAL and call(entry, vocab=1025) == EINVAL and call(entry, state=None) == EINVAL
    entry = "cvx_t2s_beam_guided_queue_steps"
    assert call(entry, bqueue=False) == EINVAL
    assert call(entry, qstruct_size=qsize - 8) == EINVAL and call(entry, qstruct_size=qsize + 8) == EINVAL and call(entry, qstruct_size=0) == EINVAL
    for k in qnames:
        assert call(entry, qnull=k) == EINVAL, k
    assert call(entry, n_utterances=0) == EINVAL and call(entry, n_utterances=-1) == EINVAL
    # the unguided entry points still refuse guidance
    assert call("cvx_t2s_beam_steps", cfg_scale=1.5) == EINVAL and call("cvx_t2s_beam_queue_steps", cfg_scale=1.5) == EINVAL
    assert torch.equal(model.buf["state"], sentinel) and torch.equal(bm["groups"], groups)
    assert torch.equal(bq["utterances"], utter) and torch.equal(bq["queue"], queue)
    assert bool((bm["scores"] == -3.0).all()) and bool((bm["logprobs"] == 7.0).all())
    assert bool((bq["logprobs"] == 7.0).all()) and bool((bq["final_scores"] == 9.0).all())
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- 14. the facade
def test_facade_guided_beam_search(decoder):
    from covomix_amd.conditional_model import CoVoMixModel
    g, sd, model = decoder
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval().to(DEV)
    ids = _texts(g, 3, seed=9)
    kw = dict(beam_search_decode=True, beam_size=4, max_length=24, cond_scale=1.5, guided_beam=True)
    want = [model.generate_beam(i_, beam_size=4, max_length=24, cond_scale=1.5) for i_ in ids]
    flat = m.synthesis_sample_text2semantic(ids[0].to(DEV), **kw)
    assert flat.device.type == "cuda" and torch.equal(flat.cpu(), want[0][0])
    full = m.synthesis_sample_text2semantic(ids[0], return_logprobs=True, **kw)
    assert len(full) == 3 and all(torch.equal(a, b) for a, b in zip(full, want[0][:3]))
    lst = m.synthesis_sample_text2semantic(ids, **kw)
    assert len(lst) == 3 and all(torch.equal(a, w[0]) for a, w in zip(lst, want))
    lst = m.synthesis_sample_text2semantic(ids, return_logprobs=True, **kw)
    assert all(torch.equal(a[2], w[2]) for a, w in zip(lst, want))
    ten = m.synthesis_sample_text2semantic(ids[0], beam_search_decode=True, max_length=24, cond_scale=1.5, guided_beam=True)   # default: 10
    assert torch.equal(ten, model.generate_beam(ids[0], beam_size=10, max_length=24, cond_scale=1.5)[0])
    pen = m.synthesis_sample_text2semantic(ids[0], length_penalty=0.0, return_logprobs=True, **kw)
    assert torch.equal(pen[1], model.generate_beam(ids[0], beam_size=4, max_length=24, length_penalty=0.0, cond_scale=1.5)[1])
    # the switch with scale 1 is the plain beam call
    plain = m.synthesis_sample_text2semantic(ids[0], beam_search_decode=True, beam_size=4, max_length=24, guided_beam=True)
    assert torch.equal(plain, model.generate_beam(ids[0], beam_size=4, max_length=24)[0])
    # the pinned refusals, without the switch
    off = {k: v for k, v in kw.items() if k != "guided_beam"}
    with pytest.raises(NotImplementedError, match="guidance"):
        m.synthesis_sample_text2semantic(ids[0], **off)
    with pytest.raises(NotImplementedError, match="guidance"):
        m.synthesis_sample_text2semantic(ids, **off)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], best_of=2, **kw)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], uniforms=torch.rand(24, 1, model.d["vocab"]), **kw)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids, **{**kw, "cond_scale": [1.5, 2.0, 1.5]})


# ---------------------------------------------------------------- 15. the CLI flag
def test_cli_beam_guided(tmp_path, monkeypatch):
    """a two-turn dialogue: --t2s_beam_size 4 --t2s_cond_scale 1.5 --t2s_beam_guided runs the guided beam search per turn and writes the
    files; without the last flag the combination is refused as before"""
    import covomix_amd.synthetic as syn
    from covomix_amd import generation
    from test_generation_gpu import _write_fixture
    tmp = str(tmp_path)
    _write_fixture(tmp, "vosingle")
    shapes = syn.t2s_param_shapes(two_output=False, dim=64, dim_target=64, source_depth=2, target_depth=2, heads=1, num_text=200)
    tsd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=0).items()}
    torch.save({"state_dict": {"cfm_wrapper.model." + k: v for k, v in tsd.items()},
                "hyper_parameters": {"text2semantic": True, "cond_drop_prob": 0.25}}, os.path.join(tmp, "t2s.ckpt"))
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
        seen.append((kw.get("beam_search_decode", False), kw.get("beam_size"), kw.get("cond_scale"), kw.get("guided_beam"), "uniforms" in kw,
                     len(ids)))
        return real(self, ids, max_length=12, **kw)
    monkeypatch.setattr(generation.CoVoMixModel, "synthesis_sample_text2semantic", spy)
    base = ["--t2s_ckpt", os.path.join(tmp, "t2s.ckpt"), "--acous_ckpt", os.path.join(tmp, "acous.ckpt"),
            "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"), "--text_dir", tdir, "--prompt_dir", pdir, "--mode", "covosingle"]
    flags = ["--t2s_beam_size", "4", "--t2s_cond_scale", "1.5"]
    with pytest.warns(UserWarning, match="EMA"):
        assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, "o0")] + flags + ["--t2s_beam_guided"]) == 1
    files = sorted(os.listdir(os.path.join(tmp, "o0")))
    assert "dlg_a.wav" in files
    assert seen == [(True, 4, 1.5, True, False, 2)]
    with pytest.raises(ValueError, match="t2s_beam_size"):
        generation.run(True, base + ["--saved_dir", os.path.join(tmp, "o1")] + flags)
    assert len(seen) == 1
