"""GPU: text2semantic beam search through continuously refilled slot groups (cvx_t2s_beam_queue_steps,
TextToSemanticDecoder.generate_beam_many).  The contract is bit-identity with generate_beam of the utterance alone: every comparison is
torch.equal / ==.

  1. refilled == alone: seven texts, per-utterance limits (odd and even ends, one on a CHUNK boundary, one of a single step), beam sizes
     3 / 10 / 16 on 3 / 2 / 4 groups - and some group decoded at least two utterances;
  2. after a refill every hypothesis' log-probs == its teacher-forced score (the indirect attention read the new utterance's rows only,
     the previous one's cache and owner rows still in place) - with re-parenting;
  3. groups that end because all hypotheses finished (an adjusted eos embedding row), a later utterance in the freed group;
  4. windows;  5. nothing moves for the other decode paths;  6. refusals launch nothing.
The fixtures are the committed cosingle_small / comix_small models with max_length = 40."""
import ctypes as C
import math

import pytest
import torch

import t2s_beam_restated as br
from test_t2s_filters import decode_uniforms, load_small

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
MAX_LEN = 40
NAMES = ("cosingle_small", "comix_small")
LIMITS = (5, 40, 17, 16, 33, 1, 24)            # odd / even ends, 16 = a CHUNK boundary, 1 = a single step
CASES = [(3, 9), (10, 20), (16, 64)]            # (beam size, slots): 3 groups (one across the 8-slot gemv boundary), 2 groups, 4 groups
KEYS = ("parents", "tokens", "logprobs", "lengths", "order")


@pytest.fixture(scope="module")
def decoders():
    from covomix_amd.t2s import TextToSemanticDecoder
    out = {}
    for name in NAMES:
        g, sd = load_small(name)
        out[name] = (g, sd, TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN))
    return out


def _cuts(g, n, seed):
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


def _same_hyp(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


def _same_record(a, b):
    return all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in KEYS + ("steps",)) and \
        torch.equal(a["scores"], b["scores"])


_CACHE: dict = {}


def _alone(decoders, name, B):
    """the references, computed once: (hypotheses, last_beam record) of every one of the seven utterances decoded alone"""
    key = ("alone", name, B)
    if key not in _CACHE:
        g, sd, model = decoders[name]
        ref = []
        for src, lim in zip(_cuts(g, 7, seed=21), LIMITS):
            beams = model.generate_beam(src, B, max_length=lim, return_beams=True)
            ref.append((beams, model.last_beam[0]))
        _CACHE[key] = ref
    return _CACHE[key]


def _refilled(decoders, name, B, slots):
    key = ("many", name, B, slots)
    if key not in _CACHE:
        g, sd, model = decoders[name]
        out = model.generate_beam_many(_cuts(g, 7, seed=21), B, return_beams=True, slots=slots, limits=LIMITS)
        _CACHE[key] = (out, list(model.last_beam))
    return _CACHE[key]


def _check_against_alone(out, recs, ref, B, tag):
    assert len(out) == len(recs) == len(ref) == 7
    for j in range(7):
        beams, rec = ref[j]
        assert len(out[j]) == B and all(_same_hyp(a, b) for a, b in zip(out[j], beams)), (tag, j)
        assert _same_record(recs[j], rec), (tag, j)
        # (status 2: all hypotheses finished, possibly before the limit; 3: the limit ended it)
        assert recs[j]["status"] in (2, 3) and recs[j]["steps"] <= LIMITS[j] and (recs[j]["status"] == 2 or recs[j]["steps"] == LIMITS[j]), (tag, j)


# ---------------------------------------------------------------- 1. refilled == alone
@pytest.mark.parametrize("B,slots", CASES)
@pytest.mark.parametrize("name", NAMES)
def test_refilled_equals_alone(decoders, name, B, slots):
    ref = _alone(decoders, name, B)
    out, recs = _refilled(decoders, name, B, slots)
    _check_against_alone(out, recs, ref, B, (name, B))
    groups = [r["group"] for r in recs]
    G = min(slots // B, 64 // B, 7)
    print(f"{name} B={B}: utterance -> group {groups}")
    assert all(0 <= x < G for x in groups) and groups[:G] == list(range(G))
    assert max(groups.count(x) for x in set(groups)) >= 2, "no group decoded two utterances: nothing was refilled"
    g, sd, model = decoders[name]
    best = model.generate_beam_many(_cuts(g, 7, seed=21), B, slots=slots, limits=LIMITS)
    assert all(_same_hyp(a, h[0]) for a, h in zip(best, out))


# ---------------------------------------------------------------- 2. forced scores after a refill
def _reparented(rec, slot, steps):
    """steps of the hypothesis in `slot` at which it came from another slot (test_t2s_beam_gpu._reparented_steps)"""
    from covomix_amd.t2s import beam_backtrack
    path = beam_backtrack(rec["parents"], rec["tokens"], rec["logprobs"], slot, steps)[2]
    return sum(1 for t in range(steps) if int(rec["parents"][t, path[t]]) != path[t])


@pytest.mark.parametrize("B,slots", CASES)
@pytest.mark.parametrize("name", NAMES)
def test_hypotheses_after_a_refill_equal_their_forced_score(decoders, name, B, slots):
    g, sd, model = decoders[name]
    out, recs = _refilled(decoders, name, B, slots)
    texts = _cuts(g, 7, seed=21)
    G = min(slots // B, 64 // B, 7)
    later = list(range(G, 7))                                   # utterances that a group took on the device, after another one
    srcs, targets, where = [], [], []
    most = 0
    for j in later:
        for i, (flat, streams, lp, score) in enumerate(out[j]):
            if not math.isfinite(score):                        # (a dead hypothesis has no tokens to score)
                continue
            srcs.append(texts[j]); targets.append(streams); where.append((j, i))
            slot = recs[j]["order"][i]
            most = max(most, _reparented(recs[j], slot, recs[j]["lengths"][slot]))
    assert len(targets) >= len(later) * min(B, 2)
    scored = model.score_many(srcs, targets)
    for (j, i), want in zip(where, scored):
        assert torch.equal(out[j][i][2], want), (name, B, j, i)
    print(f"{name} B={B}: a hypothesis of a refilled group changed slots at {most} steps")
    assert most >= 4, "no hypothesis of a refilled group was re-parented at four or more steps: the ancestry table was not exercised"


# ---------------------------------------------------------------- 3. groups that end by eos
@pytest.mark.parametrize("name,tok,alpha,B", [("cosingle_small", 95, 1.2, 3), ("comix_small", 400, 1.01, 3)])
def test_groups_that_end_by_eos_are_refilled(name, tok, alpha, B):
    """the adjusted-eos models of test_t2s_beam_gpu.test_finished_hypotheses_end_to_end: the full text's search ends after 5 / 3 steps"""
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_small(name)
    sd = dict(sd)
    E = sd["semantic_token_emb.weight"].clone()
    E[-1] = alpha * E[tok]
    sd["semantic_token_emb.weight"] = E
    texts = _cuts(g, 5, seed=33)
    steps = br.oracle_beam(sd, texts[0], B, MAX_LEN)
    assert steps[-1]["ended"] and len(steps) < MAX_LEN, "the oracle search does not end early"
    model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=MAX_LEN)
    out = model.generate_beam_many(texts, B, return_beams=True, slots=2 * B)
    recs = list(model.last_beam)
    print(f"{name}: oracle ends after {len(steps)} steps; statuses {[r['status'] for r in recs]}, steps {[r['steps'] for r in recs]}, "
          f"groups {[r['group'] for r in recs]}")
    assert recs[0]["status"] == 2 and recs[0]["steps"] < MAX_LEN
    assert any(r["group"] == recs[0]["group"] for r in recs[2:]), "no later utterance ran in the group that ended by eos"
    for j, src in enumerate(texts):
        beams = model.generate_beam(src, B, return_beams=True)
        assert all(_same_hyp(a, b) for a, b in zip(out[j], beams)) and len(out[j]) == B, (name, j)
        assert _same_record(recs[j], model.last_beam[0]), (name, j)
        assert recs[j]["status"] in (2, 3) and (recs[j]["status"] == 2 or recs[j]["steps"] == MAX_LEN), (name, j)


# ---------------------------------------------------------------- 4. windows
@pytest.mark.parametrize("name", NAMES)
def test_windows(decoders, name, monkeypatch):
    from covomix_amd import t2s
    g, sd, model = decoders[name]
    B, slots = 3, 9
    ref = _alone(decoders, name, B)
    monkeypatch.setattr(t2s, "WINDOW", 12)                      # 12 // 3 = 4 utterances per window: two windows
    seen = []
    real = t2s.TextToSemanticDecoder._beam_queue_window
    monkeypatch.setattr(t2s.TextToSemanticDecoder, "_beam_queue_window", lambda self, s, *a: (seen.append(len(s)), real(self, s, *a))[1])
    out = model.generate_beam_many(_cuts(g, 7, seed=21), B, return_beams=True, slots=slots, limits=LIMITS)
    assert seen == [4, 3]
    _check_against_alone(out, list(model.last_beam), ref, B, (name, "windows"))


# ---------------------------------------------------------------- 5. unused = untouched
@pytest.mark.parametrize("name", NAMES)
def test_nothing_moves_for_the_other_paths(name):
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
        beams = model.generate_beam(src, 4, return_beams=True)
        return [t.cpu() for t in one] + [t for r in many for t in r] + model.score_many([src], [one[1]]) + \
            [t for h in beams for t in h[:3]] + [torch.tensor([h[3] for h in beams])]
    before = run()
    keys = set(model._graphs)
    assert getattr(model, "_beamq", None) is None and len(keys) == 4
    res = model.generate_beam_many([src, src[:, :7], src[:, :5]], 4, slots=8)
    assert len(res) == 3 and model._beamq is not None
    added = set(model._graphs) - keys
    assert keys <= set(model._graphs) and len(added) == 1 and all(k[0] == "beamq" and k[1] == 4 for k in added)
    after = run()
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and len(before) == len(after)
    assert set(model._graphs) == keys | added
    assert _lib.load().cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- 6. refusals launch nothing
def test_beam_queue_entry_refuses_and_launches_nothing(decoders):
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
    utter = torch.full_like(bq["utterances"], 3)
    bq["utterances"].copy_(utter)
    queue = torch.tensor([4, 8], dtype=torch.int32, device=DEV)
    bq["queue"].copy_(queue)
    bm["scores"].fill_(-3.0)
    bq["logprobs"].fill_(7.0)
    bq["final_scores"].fill_(9.0)
    names = ("scores", "finished", "owner", "groups", "parents", "hist_tokens", "hist_logprobs", "short_lp", "short_tokens", "logprobs")
    qnames = ("queue", "utterances", "start", "parents", "hist_tokens", "hist_logprobs", "final_scores", "final_steps", "final_finished",
              "tokens", "logprobs")
    size, qsize = C.sizeof(_lib.T2SBeam), C.sizeof(_lib.T2SBeamQueue)
    assert qsize == 8 + 8 * len(qnames)

    def call(beam=True, bqueue=True, struct_size=size, qstruct_size=qsize, beam_size=2, hist_len=MAX_LEN, backtrack=1, null=None, qnull=None,
             n_utterances=8, **edit):
        dec = model._descriptor(1.0, edit.pop("batch", 8), edit.pop("cfg_scale", 1.0), edit.pop("queue", False), None, edit.pop("nd", 0))
        for name, v in edit.items():
            setattr(dec, name, v)
        bs = _lib.T2SBeam(struct_size, beam_size, hist_len, backtrack,
                          *[None if k == null else (bq["owner"] if k == "owner" else bm[k]).data_ptr() for k in names])
        qs = _lib.T2SBeamQueue(qstruct_size, n_utterances,
                               *[None if k == qnull else (model.start if k == "start" else bq[k]).data_ptr() for k in qnames])
        rc = lib.cvx_t2s_beam_queue_steps(C.byref(dec), C.byref(bs) if beam else None, C.byref(qs) if bqueue else None, 1, ops._stream())
        torch.cuda.synchronize()
        return rc

    assert call(beam=False) == EINVAL and call(bqueue=False) == EINVAL
    assert call(struct_size=size - 8) == EINVAL and call(struct_size=size + 8) == EINVAL and call(struct_size=0) == EINVAL
    assert call(qstruct_size=qsize - 8) == EINVAL and call(qstruct_size=qsize + 8) == EINVAL and call(qstruct_size=0) == EINVAL
    for k in names:
        assert call(null=k) == EINVAL, k
    for k in qnames:
        assert call(qnull=k) == EINVAL, k
    assert call(n_utterances=0) == EINVAL and call(n_utterances=-1) == EINVAL
    assert call(queue=True, nd=8) == EINVAL                             # the dialogue queue of the sampled decode
    assert call(cfg_scale=1.5) == EINVAL                                # guidance
    for b_ in (0, -1, 17, 3, 5):                                        # outside [1, 16], or no divisor of batch = 8
        assert call(beam_size=b_) == EINVAL, b_
    assert call(beam_size=16, batch=8) == EINVAL
    assert call(hist_len=MAX_LEN - 1) == EINVAL
    assert call(batch=65) == EINVAL and call(vocab=1025) == EINVAL and call(state=None) == EINVAL      # the inherited descriptor checks
    assert torch.equal(model.buf["state"], sentinel) and torch.equal(bm["groups"], groups)
    assert torch.equal(bq["utterances"], utter) and torch.equal(bq["queue"], queue)
    assert bool((bm["scores"] == -3.0).all()) and bool((bq["logprobs"] == 7.0).all()) and bool((bq["final_scores"] == 9.0).all())
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION
