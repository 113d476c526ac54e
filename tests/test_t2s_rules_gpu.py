"""GPU: the history rules of the text2semantic decode - repetition penalty, no-repeat n-gram, minimum length (cvx_t2s_decode_steps_rules,
cvx_t2s_rules_f32; generate / generate_batch / generate_many(..., repetition_penalty=, repetition_window=, no_repeat_ngram_size=,
min_length=), per utterance through settings=, the facade's keywords).
The checker is tests/t2s_rules_restated.py (pinned on the CPU against a brute-force loop, tests/test_t2s_rules.py, where the caps used
here - at most 5 % undecidable steps, no fallback step, and rule-free decodes that DO repeat - are shown on the CPU oracle alone).
Small fixtures, V = 502, max_length = 256, at most 64 steps per decode; decodes alone are computed once and shared."""
import ctypes as C
import itertools
from unittest import mock

import pytest
import torch

import t2s_filter_restated as fr
import t2s_rules_restated as rr
from test_t2s_filters import DECODE_STEPS, decode_uniforms, load_small
from test_t2s_filters_gpu import _texts
from test_t2s_rules import DECODE_KS, RULE_SETS, THETAS, random_row

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
NAMES = ["cosingle_small", "comix_small"]
N_QUEUE = 12
FIELDS = ("repetition_penalty", "repetition_window", "no_repeat_ngram_size", "min_length")


def kw_of(rules):
    return dict(zip(FIELDS, rules))


def topk(k):
    return dict(filter_logits_fn="top_k", filter_fn_kwargs={"k": k})


# rule sets and filter settings of the queue tests, in rotation (six and four entries over 12 utterances: twelve different pairings, and
# a rotation of the rule sets by one changes every utterance's pair)
QUEUE_RULES = list(RULE_SETS.values()) + [rr.OFF, (2.0, 4, 2, 20)]
QUEUE_FILTERS = [topk(7), topk(1), dict(temperature=0.7, filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.9}), dict(temperature=1.0)]


class Case:
    """one small model, the golden text, 12 more texts with their own draws, and decodes ALONE computed once"""

    def __init__(self, name):
        from covomix_amd.t2s import TextToSemanticDecoder
        self.name = name
        self.g, sd = load_small(name)
        self.model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=256)
        self.S, self.V = self.g["uniforms"].shape[1], self.g["uniforms"].shape[-1]
        self.src = torch.from_numpy(self.g["source_ids"])
        self.uni = decode_uniforms(self.S, self.V)
        self.srcs = _texts(self.g, N_QUEUE, seed=23)
        self.unis = [decode_uniforms(self.S, self.V, salt=500 + i) for i in range(N_QUEUE)]
        self._stepwise, self._alone = {}, {}

    def stepwise(self, k, rules):
        """(flat, streams [S, L], logits [L, S, V]) of the golden text, one launch chain per step (no graph), host tensors"""
        if (k, rules) not in self._stepwise:
            r = self.model.generate(self.src, uniforms=self.uni, max_length=DECODE_STEPS, collect_logits=True, **topk(k), **kw_of(rules))
            self._stepwise[(k, rules)] = tuple(t.cpu() for t in r)
        return self._stepwise[(k, rules)]

    def alone(self, j, fi, ri, **kw):
        """(flat, streams, logprobs) of utterance j alone with filter setting fi and rule set ri as the call's scalars"""
        key = (j, fi, ri, tuple(sorted(kw.items())))
        if key not in self._alone:
            r = self.model.generate(self.srcs[j], uniforms=self.unis[j], max_length=DECODE_STEPS, return_logprobs=True, **QUEUE_FILTERS[fi],
                                    **kw_of(QUEUE_RULES[ri]), **kw)
            self._alone[key] = tuple(t.cpu() for t in r)
        return self._alone[key]


@pytest.fixture(scope="module")
def cases():
    return {n: Case(n) for n in NAMES}


def _same(res, want):
    return len(res) == len(want) == 3 and all(torch.equal(a.cpu(), b.cpu()) and a.dtype == b.dtype for a, b in zip(res, want))


# ---------------------------------------------------------------- 1. the stand-alone entry == the restatement, bit for bit
HIST_LD = 256


@pytest.mark.parametrize("V", [5, 502, 503, 1024])
def test_rules_entry_equals_restatement(V):
    """cvx_t2s_rules_f32 over the grid n in 0..8 x W in {0, 1, 7, >= len} x theta in {1, 1.3, 2, 0.5} x history lengths {0, 1, 2, n - 1,
    n, 63, 64, 65, 255, 256}, m alternating between 0 and beyond the history, rows with +-0, negative and -inf entries, histories over
    few ids (n-grams repeat), and rows whose every id is banned: the bits of tests/t2s_rules_restated.apply_rules; NaN guard bands
    around `out` stay, the inputs are not written."""
    from covomix_amd import ops
    from covomix_amd.t2s import rules_rows
    gen = torch.Generator().manual_seed(7000 + V)
    eos = V - 1
    rows = []
    for n, W, theta in itertools.product(range(9), (0, 1, 7, HIST_LD + 9), THETAS):
        for i, length in enumerate(sorted({0, 1, 2, max(n - 1, 0), n, 63, 64, 65, 255, 256})):
            m = 0 if (i + n + W) % 2 else length + 1
            rows.append(((theta, W, n, m), torch.randint(0, min(V, 6), (length,), generator=gen)))
    for n, m in ((1, 0), (1, 300), (2, 0)):                      # every id of a small alphabet seen (n = 1: all banned; V = 5: the fallback)
        rows.append(((2.0, 0, n, m), torch.arange(5).repeat(4) % V))
    R = len(rows)
    logits = torch.stack([random_row(gen, V) for _ in range(R)])
    hist = torch.full((R, HIST_LD), -7, dtype=torch.int64)       # (behind hist_len: never read - a read id of -7 would mark nothing, a compare would differ)
    for r, (_, h) in enumerate(rows):
        hist[r, :h.numel()] = h
    hlen = torch.tensor([h.numel() for _, h in rows], dtype=torch.int32)
    table = rules_rows([ru for ru, _ in rows])
    d_logits, d_hist, d_hlen, d_table = (t.to(DEV) for t in (logits, hist, hlen, table))
    guard = torch.full(((R + 2) * V,), float("nan"), device=DEV)
    out = guard[V:(R + 1) * V].view(R, V)
    got = ops.t2s_rules(d_logits, d_hist, d_hlen, d_table, eos, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool(torch.isnan(guard[:V]).all()) and bool(torch.isnan(guard[(R + 1) * V:]).all())
    assert torch.equal(d_logits.cpu().view(torch.int32), logits.view(torch.int32)) and torch.equal(d_hist.cpu(), hist)
    assert torch.equal(d_hlen.cpu(), hlen) and torch.equal(d_table.cpu(), table)
    got = got.cpu()
    voids = 0
    for r, (ru, h) in enumerate(rows):
        want, void = rr.apply_rules(logits[r], h, ru, eos)
        voids += int(void)
        assert torch.equal(got[r].view(torch.int32), want.view(torch.int32)), (V, r, ru, h.numel(), int((got[r] != want).sum()))
    print("V", V, "rows", R, "fallback rows", voids)
    assert voids >= (2 if V == 5 else 0)
    # a fresh allocation through the wrapper gives the same rows
    assert torch.equal(ops.t2s_rules(d_logits, d_hist, d_hlen, d_table, eos).cpu().view(torch.int32), got.view(torch.int32))


# ---------------------------------------------------------------- 2. the decode under rules == the restatement on its own logits
@pytest.mark.parametrize("rules", list(RULE_SETS))
@pytest.mark.parametrize("k", DECODE_KS)
@pytest.mark.parametrize("name", NAMES)
def test_ruled_decode_equals_restatement(cases, name, k, rules):
    """generate(collect_logits=True) under a rule set: at every decidable step the token of restated_decode_choice on the GPU's own
    (pre-rule) logits with the GPU's own history; at most 5 % undecidable steps, no fallback step (both caps: tests/test_t2s_rules.py);
    no n-gram twice in a stream, no eos below m; the result differs from the rule-free decode; the graph replay gives the same streams.
    (min_length alone cannot change a decode that samples no eos in 64 steps - k = 7 and k = 1 do not: for that rule set the
    difference is shown on cosingle_small under the default filter, which ends at step 18 without it.)"""
    c = cases[name]
    ru = RULE_SETS[rules]
    theta, W, n, m = ru
    flat, streams, logits = c.stepwise(k, ru)
    L = streams.shape[1]
    assert logits.shape == (L, c.S, c.V)
    tokens, decidable, fallbacks = rr.restated_decode_choice(logits, c.uni, (1.0, fr.TOP_K, k, 0.0), ru, tokens=streams.T)
    bad = int((~decidable).sum())
    print(name, k, rules, "steps", L, "undecidable", bad, "fallbacks", fallbacks)
    assert torch.equal(tokens[decidable], streams.T[decidable])
    assert bad <= 0.05 * decidable.numel() and fallbacks == 0
    for s in range(c.S):
        if n:
            assert rr.repeated_ngrams(streams[s], n) == 0, (name, k, rules, s)
        if m:
            assert L >= m and not bool((streams[s, :m] == c.V - 1).any())
    free = c.stepwise(k, rr.OFF)
    assert all(rr.repeated_ngrams(free[1][s], 2) > 0 for s in range(c.S))        # (the decode the rules are there for)
    if theta != 1.0 or n:
        assert not torch.equal(free[1], streams), (name, k, rules, "changed nothing")
    elif name == "cosingle_small" and k == DECODE_KS[0]:
        short = c.model.generate(c.src, uniforms=c.uni, max_length=DECODE_STEPS, return_streams=True)[1]
        long = c.model.generate(c.src, uniforms=c.uni, max_length=DECODE_STEPS, return_streams=True, **kw_of(ru))[1]
        assert short.shape[1] < m <= long.shape[1] and not bool((long[:, :m] == c.V - 1).any())
    # the pre-rule rows are the model's: the logits of the rule-free decode as long as the two decodes agree
    Lc = min(L, free[1].shape[1])
    same = int((free[1][:, :Lc] == streams[:, :Lc]).all(dim=0).long().cumprod(0).sum())       # leading steps with equal tokens
    assert torch.equal(logits[:min(same + 1, Lc)], free[2][:min(same + 1, Lc)])
    replay = c.model.generate(c.src, uniforms=c.uni, max_length=DECODE_STEPS, return_streams=True, **topk(k), **kw_of(ru))
    assert torch.equal(replay[1].cpu(), streams) and torch.equal(replay[0].cpu(), flat)


# ---------------------------------------------------------------- 3. log-probs stay the model's
@pytest.mark.parametrize("name", NAMES)
def test_logprobs_under_rules_equal_score_many(cases, name):
    c = cases[name]
    for k, rules in ((7, "ngram3_penalty"), (1, "ngram2"), (7, "min40")):
        r = c.model.generate(c.src, uniforms=c.uni, max_length=DECODE_STEPS, return_logprobs=True, **topk(k), **kw_of(RULE_SETS[rules]))
        assert torch.equal(r[1].cpu(), c.stepwise(k, RULE_SETS[rules])[1])
        scored = c.model.score_many([c.src], [r[1].cpu()])[0]
        assert torch.equal(scored.view(torch.int32), r[2].cpu().view(torch.int32)), (name, k, rules)
        # a banned token's log-prob is still finite: the row before the rules
        assert bool(torch.isfinite(r[2]).all())


# ---------------------------------------------------------------- 4. a neutral row through the rules entry == the chain without rules
@pytest.mark.parametrize("name", NAMES)
def test_neutral_rules_equal_the_per_dialogue_chain(cases, name):
    """theta = 1, n = 0, m = 0 through cvx_t2s_decode_steps_rules (the host forced onto the rules chain): the tokens and log-probs of the
    per-dialogue chain, bit for bit - without a queue (generate) and with one (generate_many through refilled slots)"""
    from covomix_amd import t2s
    c = cases[name]
    m = c.model
    sets = [QUEUE_FILTERS[j % 4] for j in range(6)]
    plain_one = m.generate(c.src, uniforms=c.uni, max_length=DECODE_STEPS, return_logprobs=True, **topk(7))
    plain_many = m.generate_many(c.srcs[:6], c.unis[:6], max_length=DECODE_STEPS, slots=4, return_logprobs=True, settings=sets)
    with mock.patch.object(t2s, "rules_active", lambda resolved: True):
        ruled_one = m.generate(c.src, uniforms=c.uni, max_length=DECODE_STEPS, return_logprobs=True, **topk(7))
        ruled_many = m.generate_many(c.srcs[:6], c.unis[:6], max_length=DECODE_STEPS, slots=4, return_logprobs=True, settings=sets)
    assert any(k_[-1] == "rules" for k_ in m._graphs), "the rules chain did not run"
    assert _same(ruled_one, plain_one)
    for j in range(6):
        assert _same(ruled_many[j], plain_many[j]), (name, j)


# ---------------------------------------------------------------- 5. rule sets and filters in rotation through refilled slots
@pytest.mark.parametrize("slots", [1, 8, 16])
@pytest.mark.parametrize("name", NAMES)
def test_rotating_rules_equal_alone(cases, name, slots):
    """12 utterances, six rule sets and four filter settings in rotation, through 1 / 8 / 16 slots: every utterance == its decode alone
    with its rules and settings as the call's scalars - tokens, streams, log-probs.  A refilled slot names a new dialogue, whose token row
    is its history: nothing is inherited.  12 utterances cannot reuse each of 8 slots, so: at 8 slots every slot is used and the four
    utterances behind the first eight run in slots that held another one, at 1 slot all eleven do; at 8 slots once more with the rule
    sets rotated by one against the utterances (a table indexed by the slot would survive the first run).  One graph serves every mix."""
    c = cases[name]
    m = c.model
    for rot in ((0, 1) if slots == 8 else (0,)):
        pick = [(j % len(QUEUE_FILTERS), (j + rot) % len(QUEUE_RULES)) for j in range(N_QUEUE)]
        want = [c.alone(j, *pick[j]) for j in range(N_QUEUE)]
        sets = [dict(QUEUE_FILTERS[fi], **kw_of(QUEUE_RULES[ri])) for fi, ri in pick]
        res = m.generate_many(c.srcs, c.unis, max_length=DECODE_STEPS, slots=slots, return_logprobs=True, settings=sets)
        rec = m.last_records
        for j in range(N_QUEUE):
            assert _same(res[j], want[j]), (name, slots, rot, j, pick[j], rec[j])
        used = [rec[j][5] for j in range(N_QUEUE)]
        if slots == 8:
            assert len(set(used)) == 8 and len(used) - len(set(used)) == 4
        if slots == 1:
            assert set(used) == {0}
    assert sum(1 for k_ in m._graphs if k_[0] == "per" and k_[-1] == "rules" and k_[4]) <= 3      # (queue graphs: one per slot count)
    if slots == 8:
        # the rules arrive: an utterance under a rule set differs from itself without (same filter), for at least one utterance per set
        # (a minimum length alone changes only a decode that samples an early eos: test_ruled_decode_equals_restatement shows that one)
        for ri, ru in enumerate(QUEUE_RULES):
            if ru[0] != 1.0 or ru[2]:
                mine = [j for j in range(N_QUEUE) if j % len(QUEUE_RULES) == ri]
                assert any(not torch.equal(c.alone(j, j % 4, ri)[1], c.alone(j, j % 4, QUEUE_RULES.index(rr.OFF))[1]) for j in mine), (name, ru)
        # scalars for the call, an entry overriding one field
        part = m.generate_many(c.srcs[:3], c.unis[:3], max_length=DECODE_STEPS, slots=2, return_logprobs=True, **QUEUE_FILTERS[0],
                               **kw_of(QUEUE_RULES[1]), settings=[None, kw_of(QUEUE_RULES[2]), {"temperature": 1.0}])
        assert _same(part[0], c.alone(0, 0, 1)) and _same(part[1], c.alone(1, 0, 2)) and _same(part[2], c.alone(2, 0, 1))


# ---------------------------------------------------------------- 6. guidance: slot pairs, and the mixed pool
def test_guided_and_mixed_equal_alone(cases):
    """cosingle_small under guidance (the scale of the cfg fixture's family, 2.0): four guided utterances with rotating rule sets through two
    slot pairs, and one mixed_guidance call of guided and unguided utterances - each equals its decode alone.  The history of a pair is the
    text record's token row; the rules act on the guidance-combined row."""
    c = cases["cosingle_small"]
    m = c.model
    n = 6
    ris = [j % len(QUEUE_RULES) for j in range(n)]
    guided = [c.alone(j, 0, ris[j], cond_scale=2.0) for j in range(n)]
    res = m.generate_many(c.srcs[:4], c.unis[:4], max_length=DECODE_STEPS, slots=4, cond_scale=2.0, return_logprobs=True, **QUEUE_FILTERS[0],
                          settings=[kw_of(QUEUE_RULES[ris[j]]) for j in range(4)])
    for j in range(4):
        assert _same(res[j], guided[j]), ("pairs", j)
    assert not torch.equal(guided[1][1], c.alone(1, 0, ris[1])[1])                       # (guidance itself changes the decode)
    assert not torch.equal(guided[0][1], c.alone(0, 0, QUEUE_RULES.index(rr.OFF), cond_scale=2.0)[1])
    scales = [1.0, 2.0, 2.0, 1.0, 2.0, 1.0]
    mixed = m.generate_many(c.srcs[:n], c.unis[:n], max_length=DECODE_STEPS, slots=4, return_logprobs=True, mixed_guidance=True, **QUEUE_FILTERS[0],
                            settings=[dict(kw_of(QUEUE_RULES[ris[j]]), cond_scale=scales[j]) for j in range(n)])
    for j in range(n):
        want = guided[j] if scales[j] > 1 else c.alone(j, 0, ris[j])
        assert _same(mixed[j], want), ("mixed", j, scales[j], m.last_records[j])
    scored = m.score_many([c.srcs[1]], [guided[1][1]], cond_scale=2.0)[0]
    assert torch.equal(scored.view(torch.int32), guided[1][2].view(torch.int32))


# ---------------------------------------------------------------- 7. a prefix is history
@pytest.mark.parametrize("name", NAMES)
def test_prefix_continuation_under_rules(cases, name):
    """a prefix cut from a ruled result at P in {1, n - 1, 17} (n = 3), with the same draws and rules, reproduces the rest - the n-grams
    and the penalty reach across the boundary - and the log-probs of the whole row"""
    c = cases[name]
    ru = RULE_SETS["ngram3_penalty"]
    kw = dict(max_length=DECODE_STEPS, return_logprobs=True, **topk(7), **kw_of(ru))
    A = tuple(t.cpu() for t in c.model.generate(c.src, uniforms=c.uni, **kw))
    assert torch.equal(A[1], c.stepwise(7, ru)[1]) and A[1].shape[1] > 17
    for P in (1, ru[2] - 1, 17):
        B = c.model.generate_many([c.src], [c.uni], slots=1, prefixes=[A[1][:, :P]], **kw)[0]
        assert _same(B, A), (name, P)
    # the boundary matters: with the rules off behind the same prefix the decode goes elsewhere
    off = c.model.generate_many([c.src], [c.uni], slots=1, prefixes=[A[1][:, :17]], max_length=DECODE_STEPS, return_logprobs=True, **topk(7))[0]
    assert not torch.equal(off[1], A[1])


# ---------------------------------------------------------------- 8. refusals, beam search, the facade
def test_refusals_launch_nothing(cases):
    from covomix_amd import _lib, ops
    c = cases["cosingle_small"]
    m, lib = c.model, _lib.load()
    m._ensure(8, 8, 16, True)
    sentinel = torch.full_like(m.buf["state"], 5)          # position 5: a launch would advance it and write a token
    m.buf["state"].copy_(sentinel)
    m.buf["tokens"].fill_(3)
    size = C.sizeof(_lib.T2SRules)
    per = _lib.T2SPerDialogue(C.sizeof(_lib.T2SPerDialogue), m.buf["per"].shape[0], m.buf["per"].data_ptr())
    mixed = _lib.T2SMixed(C.sizeof(_lib.T2SMixed), 0)

    def rules(n_records=None, size_=size, table=True):
        t = m.buf["rules"]
        return _lib.T2SRules(size_, t.shape[0] if n_records is None else n_records, t.data_ptr() if table else None)

    def call(ru, per_=per, mx=None, scoring=None, **edit):
        dec = m._descriptor(1.0, edit.pop("batch", 8), edit.pop("cfg_scale", 1.0), edit.pop("queue", False), None, edit.pop("nd", 0))
        for k_, v in edit.items():
            setattr(dec, k_, v)
        rc = lib.cvx_t2s_decode_steps_rules(C.byref(dec), None if scoring is None else C.byref(scoring), None if per_ is None else C.byref(per_),
                                            None if mx is None else C.byref(mx), None if ru is None else C.byref(ru), 1, ops._stream())
        torch.cuda.synchronize()
        return rc

    assert call(rules(size_=size - 4)) == EINVAL and call(rules(size_=size + 8)) == EINVAL and call(rules(size_=0)) == EINVAL
    assert call(None) == EINVAL and call(rules(table=False)) == EINVAL
    assert call(rules(n_records=0)) == EINVAL
    assert call(rules(n_records=7)) == EINVAL                               # fewer rows than slots, without a queue
    assert call(rules(n_records=7), queue=True, nd=8) == EINVAL             # ... than dialogue records
    # what the underlying entries refuse
    assert call(rules(), per_=None) == EINVAL
    assert call(rules(), per_=_lib.T2SPerDialogue(C.sizeof(_lib.T2SPerDialogue), 7, m.buf["per"].data_ptr())) == EINVAL
    assert call(rules(), batch=65) == EINVAL and call(rules(), state=None) == EINVAL
    assert call(rules(), scoring=_lib.T2SScoring(16, m.max_length, None)) == EINVAL
    assert call(rules(), mx=mixed) == EINVAL                                # the mixed chain needs the queue
    assert call(rules(), mx=_lib.T2SMixed(4, 0), queue=True, nd=8) == EINVAL
    assert call(rules(), mx=_lib.T2SMixed(C.sizeof(_lib.T2SMixed), 5), queue=True, nd=8) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(m.buf["state"], sentinel) and bool((m.buf["tokens"] == 3).all())
    # a valid call on idle slots launches and writes nothing either
    m.buf["state"].copy_(m._slot_records([]))
    assert call(rules()) == 0 and bool((m.buf["tokens"] == 3).all())
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION


def test_beam_refuses_rules_and_host_validation(cases):
    c = cases["cosingle_small"]
    m = c.model
    for kw in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_length=4)):
        with pytest.raises(ValueError, match="beam search"):
            m.generate_beam(c.src, beam_size=2, max_length=8, **kw)
        with pytest.raises(ValueError, match="beam search"):
            m.generate_beam_many([c.src], beam_size=2, max_length=8, **kw)
    m.generate_beam(c.src, beam_size=2, max_length=4, repetition_penalty=1.0, repetition_window=5)      # (every rule off)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_window=-1), dict(no_repeat_ngram_size=9), dict(min_length=DECODE_STEPS + 1)):
        with pytest.raises(ValueError):
            m.generate(c.src, uniforms=c.uni, max_length=DECODE_STEPS, **kw)
        with pytest.raises(ValueError):
            m.generate_many([c.src], [c.uni], max_length=DECODE_STEPS, settings=[kw])
    # every rule off: the call as it was - no rules table in play, no "per" graph, the same graph keys
    m._graphs.clear()
    a = m.generate_many(c.srcs[:3], c.unis[:3], max_length=DECODE_STEPS, slots=2, repetition_penalty=1.0, repetition_window=9)
    b = m.generate_many(c.srcs[:3], c.unis[:3], max_length=DECODE_STEPS, slots=2)
    assert len(m._graphs) == 1 and not any("rules" in k_ or k_[0] == "per" for k_ in m._graphs)
    assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b))
    m.generate_many(c.srcs[:3], c.unis[:3], max_length=DECODE_STEPS, slots=2, settings=[{"temperature": 0.7}, None, None])
    assert [k_[-1] == "rules" for k_ in m._graphs if k_[0] == "per"] == [False]


@pytest.mark.parametrize("name", NAMES)
def test_facade_lists_equal_one_by_one(cases, name):
    from covomix_amd.conditional_model import CoVoMixModel
    c = cases[name]
    g, sd = load_small(name)
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval().to(DEV)
    ids, us = c.srcs[:3], [u[:40] for u in c.unis[:3]]
    pen, win, ng, ml = [1.3, 1.0, 2.0], [16, 0, 4], [0, 2, 3], [0, 0, 20]
    one = [m.synthesis_sample_text2semantic(ids[j], uniforms=us[j], return_logprobs=True, filter_fn_kwargs={"k": 7}, repetition_penalty=pen[j],
                                            repetition_window=win[j], no_repeat_ngram_size=ng[j], min_length=ml[j]) for j in range(3)]
    lst = m.synthesis_sample_text2semantic(ids, uniforms=us, return_logprobs=True, filter_fn_kwargs={"k": 7}, slots=2, repetition_penalty=pen,
                                           repetition_window=win, no_repeat_ngram_size=ng, min_length=ml)
    for j in range(3):
        assert _same(lst[j], one[j]), (name, j)
    free = m.synthesis_sample_text2semantic(ids, uniforms=us, return_logprobs=True, filter_fn_kwargs={"k": 7}, slots=2)
    assert any(not torch.equal(free[j][1], one[j][1]) for j in range(3))
    # scalars for a list of texts, and all-equal lists as their scalar
    sc = m.synthesis_sample_text2semantic(ids, uniforms=us, filter_fn_kwargs={"k": 7}, no_repeat_ngram_size=2)
    eq = m.synthesis_sample_text2semantic(ids, uniforms=us, filter_fn_kwargs={"k": 7}, no_repeat_ngram_size=[2, 2, 2])
    assert all(torch.equal(a, b) for a, b in zip(sc, eq)) and torch.equal(sc[1], one[1][0])
    for bad in (dict(no_repeat_ngram_size=2), dict(min_length=[0, 1, 2]), dict(repetition_penalty=1.3)):
        with pytest.raises(ValueError):
            m.synthesis_sample_text2semantic(ids, beam_search_decode=True, beam_size=2, **bad)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], uniforms=us[0], no_repeat_ngram_size=[2])
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids, uniforms=us, no_repeat_ngram_size=9)
