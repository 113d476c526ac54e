"""GPU: beam search under the history rules no-repeat n-gram and minimum length (cvx_t2s_beam_rules_steps, cvx_t2s_beam_select_rules_f32,
TextToSemanticDecoder.generate_beam / generate_beam_many with beam_rules=True; the definition: include/covomix_hip.h).

  5. the selection entry against the fp64 restatement (tests/t2s_beam_rules_restated.py) on crafted blocks and histories - parents, tokens
     and flags exactly, token log-probs within the log-prob bound and equal, bit for bit, to cvx_t2s_logprob_f32 of the same rows, scores
     their fp32 sums - with the void and the dead-slot case;
  6. a neutral table through the new entry == the plain chain, bit for bit, lock-step and refilled, both fixtures and guided;
  7. beam_size 1 under the rules == the greedy sampled decode under the same rules;
  8. no returned hypothesis repeats an n-gram or ends below min_length, the same call without rules does; log-probs == score_many,
     scores == their fp32 sums; the search re-parents and runs odd and even steps;
  9. the search against the fp64 oracle search over the decidable prefixes of tests/test_t2s_beam_rules.py's cases;
 10. utterances with different rule rows == each alone: one wave, generate_beam_many, refilled groups (the successor's first choice is in
     its predecessor's history);
 11. past 1024 positions: the gather's stride loop wraps;
 12. refusals launch nothing; 13. the facade and the command line, with a side file.
The fixtures are the committed cosingle_small / comix_small models with max_length = 40."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import t2s_beam_restated as br
import t2s_beam_rules_restated as rr
import t2s_geometry as tg
import t2s_logprob_restated as rs
from test_t2s_filters import decode_uniforms, load_small

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
MAX_LEN = rr.MAX_LEN
NAMES = ("cosingle_small", "comix_small")
CONFIGS = [("cosingle_small", 1.0), ("comix_small", 1.0), ("cosingle_small", 1.5)]          # (fixture, guidance scale)
IDS = [f"{n}-{s}" for n, s in CONFIGS]


@pytest.fixture(scope="module")
def decoders():
    from covomix_amd.t2s import TextToSemanticDecoder
    out = {}
    for name in NAMES:
        g, sd = load_small(name)
        out[name] = (g, sd, TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN))
    return out


def _texts(g, n, seed):
    src = torch.from_numpy(g["source_ids"])
    gen = torch.Generator().manual_seed(seed)
    L = src.shape[1]
    out = []
    for i in range(n):
        a = int(torch.randint(0, max(1, L // 2), (1,), generator=gen))
        e = int(torch.randint(a + 3, L + 1, (1,), generator=gen))
        out.append(src[:, a:e])
    return out


def _fp32_score(lp):
    c = torch.zeros((), dtype=torch.float32)
    for t in range(lp.shape[1]):
        c = c + lp[0, t] if lp.shape[0] == 1 else c + (lp[0, t] + lp[1, t])
    return float(c)


def _same_hyp(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


def _same_record(a, b):
    return a["steps"] == b["steps"] and a["order"] == b["order"] and a["lengths"] == b["lengths"] and torch.equal(a["scores"], b["scores"]) and \
        all(torch.equal(a[k], b[k]) for k in ("parents", "tokens", "logprobs"))


def _table(G, n, m):
    t = torch.zeros(G, 4, dtype=torch.int32)
    t[:, 0] = torch.tensor(1.0).view(torch.int32)
    t[:, 2], t[:, 3] = n, m
    return t


def _reparents(rec):
    """steps at which a live hypothesis continues from another slot"""
    par, tok = rec["parents"], rec["tokens"]
    return sum(1 for t in range(rec["steps"]) if any(int(par[t, i]) != i and int(tok[t, i, 0]) >= 0 for i in range(par.shape[1])))


# ---------------------------------------------------------------- 5. the selection entry
def _check_select(lg, sc, fin, B, h, hl, table, what):
    from covomix_amd import ops
    rows, S, V = lg.shape
    ref = rr.select(lg, sc, fin, B, h, hl, table, torch.float64)
    par, tok, lp, out, ofin = (t.cpu() for t in ops.t2s_beam_select_rules(lg.to(DEV), sc.to(DEV), fin.to(DEV), B, h.to(DEV), hl.to(DEV),
                                                                         table.to(DEV)))
    assert torch.equal(par, ref["parents"]) and torch.equal(tok, ref["tokens"]) and torch.equal(ofin, ref["finished"]), what
    assert bool(((lp.double() - ref["token_lp"]).abs() <= rs.bound(ref["token_lp"])).all()), what
    base = (torch.arange(rows) // B) * B
    src_row = base + par.long()
    c = sc[src_row]
    want = torch.where(tok[:, 0] >= 0, c + lp[:, 0] if S == 1 else c + (lp[:, 0] + lp[:, 1]), c)
    want = torch.where(ref["scores"] > -math.inf, want, torch.full_like(want, -math.inf))          # dead slots
    assert torch.equal(out, want), what
    new = tok[:, 0] >= 0                                                  # the log-probs are the model's: the log-prob entry's bits
    if bool(new.any()):
        rows_lg = lg[src_row[new]].reshape(-1, V).to(DEV)
        model_lp = ops.t2s_logprob(rows_lg, tok[new].reshape(-1).to(DEV)).cpu().reshape(-1, S)
        assert torch.equal(model_lp, lp[new]), what
    return ref, (par, tok, lp, out, ofin)


HIST_KINDS = 8            # 0, n - 2, n - 1, n, 1023, 1024, 1025, 4096


def _hist_len(kind, n):
    return max(0, (0, n - 2, n - 1, n, 1023, 1024, 1025, 4096)[kind])


@pytest.mark.parametrize("V", br.VOCABS)
def test_select_rules_entry_against_the_restatement(V):
    """every B, S and history length; n and m rotate so that every (history length, n), (history length, m) and (n, m) pair occurs for
    every V.  A crafted history bans the entries the unruled selection would take first (history_block)."""
    from covomix_amd import ops
    vi = br.VOCABS.index(V)
    seen, changed = set(), 0
    for bi, B in enumerate(br.BEAMS):
        for si, S in enumerate((1, 2)):
            lg, sc, fin = br.block(B, S, V)
            rows = 3 * B
            plain = [t.cpu() for t in ops.t2s_beam_select(lg.to(DEV), sc.to(DEV), fin.to(DEV), B)]
            for kind in range(HIST_KINDS):
                n = (1, 2, 8)[(kind + bi + si) % 3]
                pos = _hist_len(kind, n)
                m = (0, pos, pos + 1)[(kind // 3 + kind + bi + vi) % 3]
                seen |= {("hn", kind, n), ("hm", kind, m - pos if m else -9), ("nm", n, m - pos if m else -9)}
                hl = torch.full((rows,), pos, dtype=torch.int32)
                for seed in range(32):                                  # before any device result is looked at
                    h = rr.history_block(B, S, V, pos, n, seed=seed)
                    if rr.decidable(lg, sc, fin, B, h, hl, _table(3, n, m)):
                        break
                else:
                    raise AssertionError(f"no decidable history for {(B, S, V, pos, n, m)}")
                ref, got = _check_select(lg, sc, fin, B, h, hl, _table(3, n, m), (B, S, V, pos, n, m))
                changed += int(not torch.equal(got[1], plain[1]))
                neutral = [t.cpu() for t in ops.t2s_beam_select_rules(lg.to(DEV), sc.to(DEV), fin.to(DEV), B, h.to(DEV), hl.to(DEV),
                                                                      _table(3, 0, 0).to(DEV))]
                assert all(torch.equal(a, b) for a, b in zip(neutral, plain)), (B, S, V, pos)
    assert len({k for k in seen if k[0] == "hn"}) == HIST_KINDS * 3 and len({k for k in seen if k[0] == "nm"}) == 9
    print(f"V = {V}: the rules changed the selected tokens in {changed} of {len(br.BEAMS) * 2 * HIST_KINDS} blocks")
    assert changed >= (8 if V > 1 else 0)


@pytest.mark.parametrize("V,n", [(3, 1), (3, 2), (5, 2), (5, 8), (502, 1), (502, 8)])
def test_select_rules_void_bans_and_dead_slots(V, n):
    """histories that ban EVERY id of [0, V - 1) (V = 502, n = 8: 4015 tokens): with the eos banned too the n-gram bans are void; with the
    eos free it is the only candidate of a live hypothesis, and the group with one live hypothesis gets B - 1 dead slots"""
    pos = rr.cover_len(V, n)
    assert pos <= 4096
    for B in br.BEAMS:
        for S in (1, 2):
            lg, sc, fin = br.block(B, S, V)
            rows = 3 * B
            h = rr.history_block(B, S, V, pos, n, kind="cover")
            hl = torch.full((rows,), pos, dtype=torch.int32)
            for m in (pos + 1, 0):
                assert rr.decidable(lg, sc, fin, B, h, hl, _table(3, n, m)), (B, S, V, n, m)
                ref, got = _check_select(lg, sc, fin, B, h, hl, _table(3, n, m), (B, S, V, n, m))
                if m:
                    assert ref["voids"] == int(((sc > -math.inf) & (fin == 0)).sum()) * S and not bool((got[1] == V - 1).any())
                else:
                    assert ref["voids"] == 0 and got[3][B + 1:2 * B].tolist() == [-math.inf] * (B - 1)
                    assert got[1][B].tolist() == [V - 1] * S and got[0][B:2 * B].tolist() == [0] + list(range(1, B))


# ---------------------------------------------------------------- 6. a neutral table == the plain chain
@pytest.mark.parametrize("name,scale", CONFIGS, ids=IDS)
def test_neutral_rules_equal_the_plain_chain(decoders, name, scale):
    from covomix_amd import ops
    g, sd, model = decoders[name]
    srcs = _texts(g, 3, seed=5)
    B = 3

    @ops.gated
    @torch.no_grad()
    def entry(fn, *args, **kw):                        # (as generate_beam / generate_beam_many call them)
        return fn(*args, **kw)
    plain = model.generate_beam(srcs, beam_size=B, return_beams=True, cond_scale=scale)
    recs = list(model.last_beam)
    model.last_beam = []
    wave = entry(model._beam_wave, srcs, B, MAX_LEN, 1.0, scale, rules=[(1.0, 0, 0, 0)] * 3)             # the new entry, lock-step
    assert any(k[-1] == "rules" for k in model._graphs)
    for j in range(3):
        assert all(_same_hyp(a, b) for a, b in zip(wave[j], plain[j])) and _same_record(model.last_beam[j], recs[j]), (name, j)
    limits = [11, 40, 7]
    plain = model.generate_beam_many(srcs, B, return_beams=True, slots=(2 if scale > 1 else 1) * B, limits=limits, cond_scale=scale)
    recs = list(model.last_beam)
    model.last_beam = []
    many = entry(model._beam_queue_window, srcs, B, limits, 1.0, (2 if scale > 1 else 1) * B, scale, rules=[(1.0, 0, 0, 0)] * 3)    # ... refilled
    for j in range(3):
        assert all(_same_hyp(a, b) for a, b in zip(many[j], plain[j])) and _same_record(model.last_beam[j], recs[j]), (name, j)
    # both rules off under the switch: the plain entries
    keys = set(model._graphs)
    off = model.generate_beam(srcs, beam_size=B, return_beams=True, cond_scale=scale, beam_rules=True)
    assert set(model._graphs) == keys and all(_same_hyp(a, b) for j in range(3) for a, b in zip(off[j], wave[j]))


# ---------------------------------------------------------------- 7. beam_size 1 == the greedy sampled decode under the same rules
@pytest.mark.parametrize("name,scale", CONFIGS, ids=IDS)
def test_beam_size_one_is_the_greedy_decode_under_the_rules(decoders, name, scale):
    g, sd, model = decoders[name]
    src = torch.from_numpy(g["source_ids"])
    S, V = model.d["streams"], model.d["vocab"]
    kw = dict(no_repeat_ngram_size=2, min_length=9)
    flat, streams, lp = model.generate(src, uniforms=decode_uniforms(S, V)[:MAX_LEN], filter_logits_fn="top_k", filter_fn_kwargs={"k": 1},
                                       return_logprobs=True, cond_scale=scale, **kw)
    bflat, bstreams, blp, score = model.generate_beam(src, beam_size=1, cond_scale=scale, beam_rules=True, **kw)
    assert torch.equal(bflat, flat.cpu()) and torch.equal(bstreams, streams.cpu())
    assert torch.equal(blp, lp.cpu()) and score == _fp32_score(blp)
    assert rr.repeats(bstreams, 2) == 0
    unruled = model.generate_beam(src, beam_size=1, cond_scale=scale)
    assert rr.repeats(unruled[1], 2) > 0 and not torch.equal(unruled[1], bstreams)


# ---------------------------------------------------------------- 8. the properties
@pytest.mark.parametrize("B", (3, 10))
@pytest.mark.parametrize("name,scale", CONFIGS, ids=IDS)
def test_no_hypothesis_breaks_a_rule_and_log_probs_stay_the_models(decoders, name, scale, B):
    g, sd, model = decoders[name]
    src = torch.from_numpy(g["source_ids"])
    V = model.d["vocab"]
    plain = model.generate_beam(src, beam_size=B, return_beams=True, cond_scale=scale)
    for n in (2, 3):
        assert sum(rr.repeats(h[1], n) for h in plain) > 0, "the search without rules does not repeat: the case shows nothing"
        for m in (0, 9, MAX_LEN):
            beams = model.generate_beam(src, beam_size=B, return_beams=True, cond_scale=scale, beam_rules=True, no_repeat_ngram_size=n,
                                        min_length=m)
            rec = model.last_beam[0]
            assert len(beams) == B and rec["steps"] >= 2 and _reparents(rec) >= 1, (name, n, m)
            alive = [h for h in beams if h[3] > -math.inf]
            assert alive
            scored = model.score_many([src] * len(alive), [h[1] for h in alive], cond_scale=scale)
            for i, (flat, streams, lp, score) in enumerate(alive):
                assert rr.repeats(streams, n) == 0 and not bool((streams[:, :m] == V - 1).any()), (name, n, m, i)
                assert torch.equal(lp, scored[i]) and score == _fp32_score(lp) == float(rec["scores"][rec["order"][i]]), (name, n, m, i)


@pytest.mark.parametrize("name,tok,alpha", [("cosingle_small", 95, 1.2), ("comix_small", 400, 1.01)])
def test_min_length_on_a_model_that_ends_early(name, tok, alpha):
    """the eos embedding row = alpha * the row of a token the greedy decode repeats (tests/test_t2s_beam_gpu.py: the hypotheses of the
    unruled search finish within five steps): under min_length = 9 none ends before step 9"""
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_small(name)
    sd = dict(sd)
    E = sd["semantic_token_emb.weight"].clone()
    E[-1] = alpha * E[tok]
    sd["semantic_token_emb.weight"] = E
    src = torch.from_numpy(g["source_ids"])
    eos = E.shape[0] - 1
    model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN)
    plain = model.generate_beam(src, beam_size=3, return_beams=True)
    assert min(h[1].shape[1] for h in plain) < 9, "the search without rules does not end early: the case shows nothing"
    beams = model.generate_beam(src, beam_size=3, return_beams=True, beam_rules=True, min_length=9)
    alive = [h for h in beams if h[3] > -math.inf]
    scored = model.score_many([src] * len(alive), [h[1] for h in alive])
    print(f"{name}: lengths without rules {[h[1].shape[1] for h in plain]}, under min_length 9 {[h[1].shape[1] for h in alive]}")
    for (flat, streams, lp, score), want in zip(alive, scored):
        assert streams.shape[1] >= 10 and not bool((streams[:, :9] == eos).any())
        assert torch.equal(lp, want) and score == _fp32_score(lp)


# ---------------------------------------------------------------- 9. against the fp64 oracle
@pytest.mark.parametrize("case", rr.ORACLE_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_against_the_oracle_beam_search_under_the_rules(decoders, case):
    """The conditions (tests/test_t2s_beam_rules.py holds them on the CPU): a decidable prefix of at least 12 steps in which the rules
    change the selection and hypotheses re-parent.  Over it: the same hypotheses - tokens, and with them every parent's tokens - and
    scores within the accumulated bound of tests/test_t2s_beam_gpu.py's comparison."""
    name, ids, B, n, m, scale = case
    g, sd, model = decoders[name]
    src_full = torch.from_numpy(g["source_ids"])
    steps, k, acc, differs, moved = rr.oracle_case(sd, src_full, case)
    assert k >= 12 and differs >= 1 and moved >= 1, "the oracle alone does not meet the conditions of this check"
    model.generate_beam(src_full[:, :ids], beam_size=B, cond_scale=scale, beam_rules=True, no_repeat_ngram_size=n, min_length=m)
    got = br.replay(*(model.last_beam[0][key] for key in ("parents", "tokens", "logprobs")))
    worst = 0.0
    for t in range(k):
        want = {h[0]: h[1] for h in steps[t]["hyps"]}
        have = {pre: float(c) for pre, c in got[t]}
        assert set(have) == set(want), (case, t)
        for pre in want:
            worst = max(worst, abs(have[pre] - want[pre]) / acc[t])
            assert abs(have[pre] - want[pre]) <= acc[t], (case, t)
    print(f"{case}: {k} steps, largest score error / accumulated bound {worst:.3f}")


# ---------------------------------------------------------------- 10. independence
NGRAMS = [1, 2, 1, 0, 3]
MINS = [0, 5, 0, 3, 0]
LIMITS = [7, 12, 5, 9, 12]


def _five(g):
    t = _texts(g, 5, seed=17)
    t[2] = t[0]                                    # the utterance that follows utterance 0 in its group decodes the same text
    return t


@pytest.mark.parametrize("name,scale", CONFIGS, ids=IDS)
def test_utterances_with_different_rules_equal_themselves_alone(decoders, name, scale):
    g, sd, model = decoders[name]
    srcs = _five(g)
    B = 3
    alone, alone_lim = [], []
    for j, src in enumerate(srcs):
        kw = dict(beam_size=B, return_beams=True, cond_scale=scale, beam_rules=True, no_repeat_ngram_size=NGRAMS[j], min_length=MINS[j])
        alone.append((model.generate_beam(src, **kw), model.last_beam[0]))
        alone_lim.append((model.generate_beam(src, max_length=LIMITS[j], **kw), model.last_beam[0]))
    assert len({tuple(a[0][0][0].tolist()) for a in alone}) > 1
    kw = dict(return_beams=True, cond_scale=scale, beam_rules=True, no_repeat_ngram_size=NGRAMS, min_length=MINS)
    wave = model.generate_beam(srcs, beam_size=B, **kw)                                            # one lock-step wave
    for j in range(5):
        assert all(_same_hyp(a, b) for a, b in zip(wave[j], alone[j][0])) and _same_record(model.last_beam[j], alone[j][1]), (name, j)
    P = 2 if scale > 1.0 else 1
    many = model.generate_beam_many(srcs, B, slots=5 * P * B, **kw)                                # a group each
    for j in range(5):
        assert all(_same_hyp(a, b) for a, b in zip(many[j], alone[j][0])) and _same_record(model.last_beam[j], alone[j][1]), (name, j)
    many = model.generate_beam_many(srcs, B, slots=2 * P * B, limits=LIMITS, **kw)                 # two groups: refilled
    recs = list(model.last_beam)
    for j in range(5):
        assert all(_same_hyp(a, b) for a, b in zip(many[j], alone_lim[j][0])) and _same_record(recs[j], alone_lim[j][1]), (name, j)
    # utterance 2 followed utterance 0 in its group, under n = 1, and takes first the token utterance 0 holds in its history
    assert recs[2]["group"] == recs[0]["group"] == 0
    first = recs[2]["tokens"][0, 0].tolist()
    assert first == recs[0]["tokens"][0, 0].tolist() and all(x >= 0 for x in first)


# ---------------------------------------------------------------- 11. past 1024 positions
def test_histories_past_1024_positions():
    from covomix_amd.t2s import TextToSemanticDecoder
    L = 1100
    model = TextToSemanticDecoder(tg.state_dict("k260-h3-v501"), torch.device(DEV), max_length=L)
    src, V = tg.text(), 501
    kw = dict(no_repeat_ngram_size=3, min_length=L)
    flat, streams, lp = model.generate(src, uniforms=tg.draws(L, 1, V, seed=3), filter_logits_fn="top_k", filter_fn_kwargs={"k": 1},
                                       return_logprobs=True, **kw)
    one = model.generate_beam(src, beam_size=1, beam_rules=True, **kw)
    assert one[1].shape == (1, L) and torch.equal(one[1], streams.cpu()) and torch.equal(one[2], lp.cpu())      # every step
    assert rr.repeats(one[1], 3) == 0
    assert rr.repeats(model.generate_beam(src, beam_size=1)[1], 3) > 0, "the decode without rules does not repeat: the case shows nothing"
    beams = model.generate_beam(src, beam_size=2, return_beams=True, beam_rules=True, **kw)
    rec = model.last_beam[0]
    assert rec["steps"] == L and _reparents(rec) >= 1
    scored = model.score_many([src] * 2, [h[1] for h in beams])
    for (flat, streams, lp, score), want in zip(beams, scored):
        assert streams.shape == (1, L) and rr.repeats(streams, 3) == 0 and not bool((streams == V - 1).any())
        assert torch.equal(lp, want) and score == _fp32_score(lp)


# ---------------------------------------------------------------- 12. refusals launch nothing
def test_rules_entries_refuse_and_launch_nothing(decoders):
    from covomix_amd import _lib, ops
    g, sd, model = decoders["cosingle_small"]
    lib = _lib.load()
    model._ensure(8, 8, 0)
    bm = model._ensure_beam()
    bq = model._ensure_beam_queue(8)
    sentinel = torch.full_like(model.buf["state"], 5)                  # position 5 of 40: a launch would advance it
    model.buf["state"].copy_(sentinel)
    groups = torch.tensor([[5, 0, MAX_LEN, 0]] * bm["groups"].shape[0], dtype=torch.int32, device=DEV)
    bm["groups"].copy_(groups)
    bm["scores"].fill_(-3.0)
    bm["short_lp"].fill_(7.0)
    bm["logprobs"].fill_(7.0)
    bq["logprobs"].fill_(7.0)
    bq["queue"].copy_(torch.tensor([2, 4], dtype=torch.int32))
    names = ("scores", "finished", "owner", "groups", "parents", "hist_tokens", "hist_logprobs", "short_lp", "short_tokens", "logprobs")
    qnames = ("parents", "hist_tokens", "hist_logprobs", "final_scores", "final_steps", "final_finished", "tokens", "logprobs")
    table = _table(8, 2, 9).to(DEV)
    rsize = C.sizeof(_lib.T2SRules)
    # EVERY buffer an entry point could write - the decode buffers, the beam state, the queue state, the table - is compared afterwards
    for pool, keys in ((bm, ("owner", "parents", "hist_tokens", "short_tokens", "finished")),
                       (bq, ("parents", "hist_tokens", "final_steps", "final_finished", "utterances", "tokens"))):
        for k in keys:
            pool[k].copy_(torch.randint(0, 3, pool[k].shape, device=DEV).to(pool[k].dtype))
    for pool, keys in ((bm, ("hist_logprobs",)), (bq, ("hist_logprobs", "final_scores"))):
        for k in keys:
            pool[k].copy_(torch.rand(pool[k].shape, device=DEV))
    pools = {"buf": model.buf, "beam": bm, "queue": bq, "rules": {"table": table}}
    before = {(p_, k): v.clone() for p_, pool in pools.items() for k, v in pool.items() if torch.is_tensor(v)}
    assert {("beam", k) for k in names} | {("queue", k) for k in qnames + ("queue", "utterances")} | {("buf", "state"), ("buf", "tokens"),
                                                                                                    ("buf", "x")} <= set(before)

    def call(queue=False, rules=True, rules_size=rsize, n_records=8, table_ptr=table.data_ptr(), beam_size=2, hist_len=MAX_LEN, n_utt=4,
             qsize=C.sizeof(_lib.T2SBeamQueue), cfg_scale=1.0, dqueue=False, beam=True, decoder=True):
        dec = model._descriptor(1.0, 8, cfg_scale, dqueue, None, 8 if dqueue else 0)
        bs = _lib.T2SBeam(C.sizeof(_lib.T2SBeam), beam_size, hist_len, 1, *[bm[k].data_ptr() for k in names])
        qs = _lib.T2SBeamQueue(qsize, n_utt, bq["queue"].data_ptr(), bq["utterances"].data_ptr(), model.start.data_ptr(),
                               *[bq[k].data_ptr() for k in qnames])
        ru = _lib.T2SRules(rules_size, n_records, table_ptr)
        rc = lib.cvx_t2s_beam_rules_steps(C.byref(dec) if decoder else None, C.byref(bs) if beam else None, C.byref(qs) if queue else None,
                                          C.byref(ru) if rules else None, 1, ops._stream())
        torch.cuda.synchronize()
        return rc

    for queue in (False, True):
        assert call(queue, rules=False) == EINVAL and call(queue, beam=False) == EINVAL and call(queue, decoder=False) == EINVAL
        assert call(queue, rules_size=rsize - 8) == EINVAL and call(queue, rules_size=rsize + 8) == EINVAL and call(queue, rules_size=0) == EINVAL
        assert call(queue, table_ptr=None) == EINVAL
        assert call(queue, n_records=0) == EINVAL and call(queue, n_records=3) == EINVAL      # 4 groups of 2 / 4 utterances
        # ... and what the plain entry of the same form refuses
        assert call(queue, beam_size=3) == EINVAL and call(queue, beam_size=17) == EINVAL and call(queue, hist_len=MAX_LEN - 1) == EINVAL
        assert call(queue, dqueue=True) == EINVAL
        assert call(queue, cfg_scale=1.5, beam_size=8) == EINVAL                               # guided: 2 * 8 slots do not divide 8
    assert call(True, n_utt=0) == EINVAL and call(True, qsize=8) == EINVAL and call(True, n_utt=9, n_records=8) == EINVAL
    assert torch.equal(model.buf["state"], sentinel) and torch.equal(bm["groups"], groups)
    assert bool((bm["scores"] == -3.0).all()) and bool((bm["logprobs"] == 7.0).all()) and bool((bm["short_lp"] == 7.0).all())
    assert bool((bq["logprobs"] == 7.0).all()) and bq["queue"].tolist() == [2, 4]
    bits = lambda t: t.contiguous().view(-1).view(torch.uint8)          # (bit for bit, whatever a float buffer holds)
    changed = [key for key, v in before.items() if not torch.equal(bits(pools[key[0]][key[1]]), bits(v))]
    assert not changed, changed
    # the selection entry
    B, S, V, ld = 2, 2, 16, 4
    lg = torch.zeros(2 * B, S, V, device=DEV)
    sc = torch.zeros(2 * B, device=DEV)
    fin = torch.zeros(2 * B, dtype=torch.uint8, device=DEV)
    h = torch.zeros(2 * B, S, ld, dtype=torch.int32, device=DEV)
    hl = torch.full((2 * B,), ld, dtype=torch.int32, device=DEV)
    tb = _table(2, 1, 0).to(DEV)
    outs = [torch.full((2 * B,), 9, dtype=torch.int32, device=DEV), torch.full((2 * B, S), 9, dtype=torch.int64, device=DEV),
            torch.full((2 * B, S), 9.0, device=DEV), torch.full((2 * B,), 9.0, device=DEV), torch.full((2 * B,), 9, dtype=torch.uint8, device=DEV)]

    def sel(groups=2, beam_size=B, streams=S, vocab=V, hist_ld=ld, null=None):
        ptr = [None if null == i else t.data_ptr() for i, t in enumerate([lg, sc, fin, h, hl, tb] + outs)]
        rc = lib.cvx_t2s_beam_select_rules_f32(*ptr[:6], groups, beam_size, streams, vocab, hist_ld, *ptr[6:], ops._stream())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(beam_size=0), dict(beam_size=17), dict(streams=0), dict(streams=3), dict(vocab=0), dict(vocab=1025), dict(groups=-1),
               dict(hist_ld=-1), dict(hist_ld=4097)):
        assert sel(**kw) == EINVAL, kw
    for i in range(11):
        assert sel(null=i) == EINVAL, i
    assert sel(groups=0) == 0
    assert all(bool((t == 9).all()) for t in outs)
    # n = 1 with id 0 in every history: token 0 is banned everywhere (without rules: tokens 0 and 1, see tests/test_t2s_beam_gpu.py)
    assert sel() == 0 and outs[1][:, 0].tolist() == [1, 1, 1, 1] and outs[1][:, 1].tolist() == [1, 2, 1, 2]
    assert sel(hist_ld=0, null=3) == 0                                   # no history at all needs no pointer
    # the host side
    src = torch.from_numpy(g["source_ids"])
    with pytest.raises(ValueError, match="beam search"):
        model.generate_beam(src, beam_size=2, beam_rules=True, repetition_penalty=1.3, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="beam search"):
        model.generate_beam_many([src], 2, beam_rules=True, repetition_penalty=1.3)
    with pytest.raises(ValueError, match="beam search"):
        model.generate_beam(src, beam_size=2, beam_rules=True, repetition_window=4, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="beam search"):
        model.generate_beam(src, beam_size=2, no_repeat_ngram_size=2)                              # without the switch: as before
    with pytest.raises(ValueError):
        model.generate_beam([src, src], beam_size=2, beam_rules=True, no_repeat_ngram_size=[2])
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- 13. the facade and the command line
@pytest.mark.parametrize("name,scale", CONFIGS, ids=IDS)
def test_facade_beam_rules(decoders, name, scale):
    from covomix_amd.conditional_model import CoVoMixModel
    g, sd, model = decoders[name]
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval().to(DEV)
    ids = _texts(g, 3, seed=9)
    kw = dict(beam_search_decode=True, beam_size=4, max_length=24, cond_scale=scale, guided_beam=scale > 1.0, beam_rules=True)
    direct = dict(beam_size=4, max_length=24, cond_scale=scale, beam_rules=True)
    want = model.generate_beam(ids[0], no_repeat_ngram_size=2, min_length=9, **direct)
    full = m.synthesis_sample_text2semantic(ids[0].to(DEV), no_repeat_ngram_size=2, min_length=9, return_logprobs=True, **kw)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(full, want[:3]))
    wants = model.generate_beam(ids, no_repeat_ngram_size=[0, 2, 3], min_length=9, **direct)
    lst = m.synthesis_sample_text2semantic(ids, no_repeat_ngram_size=[0, 2, 3], min_length=[9, 9, 9], **kw)
    assert len(lst) == 3 and all(torch.equal(a, w[0]) for a, w in zip(lst, wants))
    assert not torch.equal(lst[1], model.generate_beam(ids[1], beam_size=4, max_length=24, cond_scale=scale)[0])
    with pytest.raises(ValueError, match="beam search"):
        m.synthesis_sample_text2semantic(ids[0], repetition_penalty=1.3, **kw)
    with pytest.raises(ValueError, match="beam search"):
        m.synthesis_sample_text2semantic(ids, repetition_penalty=[1.0, 1.3, 1.0], **kw)
    with pytest.raises(ValueError, match="beam search"):
        m.synthesis_sample_text2semantic(ids, repetition_penalty=[1.3, 1.3, 1.3], no_repeat_ngram_size=2, **kw)
    for window in (4, [0, 4, 0], [4, 4, 4]):                                                         # as the command line refuses it
        with pytest.raises(ValueError, match="beam search"):
            m.synthesis_sample_text2semantic(ids, repetition_window=window, no_repeat_ngram_size=2, **kw)
    with pytest.raises(ValueError, match="beam search"):                                             # without the switch: as before
        m.synthesis_sample_text2semantic(ids[0], beam_search_decode=True, beam_size=4, no_repeat_ngram_size=2)


def test_cli_beam_rules_with_a_side_file(tmp_path, monkeypatch):
    """a two-turn dialogue under --t2s_beam_size 4 --t2s_beam_rules --t2s_no_repeat_ngram 2: turn 1 has a side file (no_repeat_ngram 3,
    min_length 5, and a temperature, which beam search ignores as before); the facade receives both turns' values and returns what the
    direct call gives"""
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
    texts = []
    for k in range(2):
        texts.append(rng.randint(1, 199, size=(1, 7 + k)).astype(np.int64))
        np.save(os.path.join(tdir, f"dlg_a.turn{k}.text_ids.npy"), texts[-1])
    with open(os.path.join(tdir, "dlg_a.turn1.t2s.json"), "w") as f:
        json.dump({"no_repeat_ngram": 3, "min_length": 5, "temperature": 0.7}, f)
    real = generation.CoVoMixModel.synthesis_sample_text2semantic
    seen = []

    def spy(self, ids, **kw):
        out = real(self, ids, max_length=12, **kw)
        seen.append((kw, [t.cpu() for t in out], self._get_t2s()))
        return out
    monkeypatch.setattr(generation.CoVoMixModel, "synthesis_sample_text2semantic", spy)
    base = ["--t2s_ckpt", os.path.join(tmp, "t2s.ckpt"), "--acous_ckpt", os.path.join(tmp, "acous.ckpt"),
            "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"), "--text_dir", tdir, "--prompt_dir", pdir, "--mode", "covosingle"]
    with pytest.warns(UserWarning, match="EMA"):
        assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, "o0"), "--t2s_beam_size", "4", "--t2s_beam_rules",
                                            "--t2s_no_repeat_ngram", "2"]) == 1
    assert len(seen) == 1
    kw, toks, dec = seen[0]
    assert kw["beam_search_decode"] and kw["beam_size"] == 4 and kw["beam_rules"] is True and "uniforms" not in kw
    assert kw["no_repeat_ngram_size"] == [2, 3] and kw["min_length"] == [0, 5]
    for k in range(2):
        want = dec.generate_beam(torch.from_numpy(texts[k]), beam_size=4, max_length=12, beam_rules=True, no_repeat_ngram_size=[2, 3][k],
                                 min_length=[0, 5][k])
        assert torch.equal(toks[k], want[0]), k
    assert "dlg_a.wav" in os.listdir(os.path.join(tmp, "o0"))
    with pytest.raises(ValueError, match="t2s_beam_size"):
        generation.run(True, base + ["--saved_dir", os.path.join(tmp, "o1"), "--t2s_beam_size", "4", "--t2s_beam_rules",
                                     "--t2s_repetition_penalty", "1.3"])
