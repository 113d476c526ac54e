"""text2semantic (CoSingle / CoMix) on the GPU - SURVEY.md section 8f row N1.

Host mirror of the reference's `TextToSemantic.generate` sampling branch + `TextToSemanticWrapper.sample`
(covomix/covomix_model/text2semantic.py:662-848, :1237-1251), the call `CoVoMixModel.synthesis_sample_text2semantic`
forwards to (covomix/conditional_model.py:313-321).  Built: the sampling branch with its three controls - temperature,
classifier-free guidance (cond_scale > 1, one-output models) and the logit filter (filter_logits_fn = top_k / top_p with
filter_fn_kwargs, text2semantic.py:118-132, :796) - in every decode schedule below; beam search (`generate_beam`: the flag the
reference's generate accepts without a body, text2semantic.py:673-677 - the algorithm is defined in include/covomix_hip.h; `generate_beam_many`:
any number of utterances through continuously refilled groups of beam_size slots); no speculative
decoding, no padded text batches.  Beside the tokens: the log-probability of every sampled token (return_logprobs), teacher-forced scoring of given tokens
through the same decode slots (score_many) and the mean token log-probability best-of-N selects by (sequence_logprob).  What is counted from
the edit distances between decoded token sequences (ops.edit_distance, csrc/edit_distance.hip): consensus selection among the candidates of
best-of-N (consensus_risks, consensus_candidate) and the reference's validation metric (token_error_rate).  And what looks at
the tokens an utterance has ALREADY emitted: the history rules - repetition penalty, no-repeat n-gram, minimum length (check_rules;
cvx_t2s_decode_steps_rules) - per utterance and per output stream, in every sampled schedule; off by default.  Under beam search
(beam_rules=True: check_beam_rules; cvx_t2s_beam_rules_steps) the last two remove candidates along every hypothesis' own ancestry.
Tokens that are already KNOWN - the targets of score_many, a forced prefix of generate_many - can take ONE causal full-sequence pass
instead of one decode step each (prefill=True, off by default: prefill_rows, _prefill; csrc/t2s_prefill.hip, cvx_t2s_prefill_attention_f32).

  encoder  (source transformer, once per utterance): the full-sequence kernels of the acoustic path - fp32 GEMM with
           the RoPE epilogue, flash attention, RMSNorm - plus a GEGLU kernel;
  decoder  (one token per step): csrc/t2s_decode.hip - cvx_t2s_decode_steps, 34 launches per step replayed from a HIP
           graph of CHUNK steps.  (Two single-launch persistent forms with grid barriers were built in round 4 and measured
           2.5-2.7x slower - a grid barrier with the L2 write-back / invalidate that cross-XCD visibility needs costs 4-7 us
           against 1.2-1.5 us for a dependent kernel boundary; removed in round 5, numbers in HISTORY.md.)  The host only
           looks at the eos flags between chunks.  `generate_batch` advances up to MAX_BATCH (64) utterances together (the
           reference decodes them one by one): a token step is a latency chain of dependent launches whose time barely
           depends on the batch, and the per-utterance arithmetic does not depend on the batch size - the tokens are
           bit-identical to the one-by-one decode.  `generate_many` decodes ANY number of utterances through a fixed number
           of decode slots with CONTINUOUS BATCHING: an utterance that has sampled its eos (text2semantic.py:803-818) frees
           its slot, and the sampling kernel of that very step hands the slot the next pending utterance (device-side
           queue, no host round trip) - real dialogues end at different steps, and a lock-step batch would run half empty.
           With mixed_guidance=True guided utterances (two slots each: text context / null context) and unguided ones (one slot)
           share that pool: a one-block scheduler launch behind the sampling kernel hands idle slots to the queue head, a guided
           utterance taking ANY two (cvx_t2s_decode_steps_mixed; `mixed_schedule` replays the policy on the host).

The reference's rotary embedding rotates interleaved pairs (2i, 2i+1) (rotary_embedding_torch.py:25-41); the kernels
rotate half-split pairs (i, i+32).  Permuting the rows of to_q and to_k inside every head (the same permutation on
both, so q.k is unchanged) maps one onto the other - done once here at load time.
"""
import ctypes as C
import math
import os
from collections.abc import Mapping
from typing import Dict, NamedTuple, Optional

import torch

from . import _lib, ops

PAD_ID = -1                    # semantic_pad_id (conditional_model.py:126)
TOP_K_THRES = 0.1              # top_k default (text2semantic.py:126)
CHUNK = 16                     # token steps per graph replay / host check
MAX_BATCH = 64                 # decode slots per step (kernel limit)
WINDOW = 256                   # utterances queued on the device at a time (generate_many)
SR = 8                         # int32 per slot / dialogue record (include/covomix_hip.h, cvx_t2s_decoder)
BEAM_MAX = 16                  # hypotheses per utterance (kernel limit)


def filter_setting(filter_logits_fn="top_k", filter_fn_kwargs=None, vocab: int = 0) -> tuple:
    """(filter mode, k, thres) of the decode descriptor from the reference's `filter_logits_fn` / `filter_fn_kwargs`
    (TextToSemantic.generate, text2semantic.py:668-669, :796).  filter_logits_fn: "top_k" or "top_p" (or a function of that name).
      top_k: kwargs `thres` (default 0.1) and `k` (default None): k = ceil(thres * vocab) unless given (:126-128); 1 <= k <= vocab.
      top_p: kwarg `thres` (default 0.9), 0 < thres < 1.  thres >= 1 is REFUSED rather than imitated: the reference compares a
             rounded fp32 cumulative sum with it, which can exceed 1 and then drops the tail of the vocabulary by rounding luck.
    ValueError outside these."""
    name = filter_logits_fn if isinstance(filter_logits_fn, str) else getattr(filter_logits_fn, "__name__", None)
    kw = dict(filter_fn_kwargs or {})
    if name == "top_k":
        thres, k = kw.pop("thres", TOP_K_THRES), kw.pop("k", None)
        if kw:
            raise ValueError(f"top_k takes thres and k, got {sorted(kw)}")
        k = math.ceil(float(thres) * vocab) if k is None else int(k)
        if not 1 <= k <= vocab:
            raise ValueError(f"top_k: k = {k} outside [1, vocab = {vocab}]")
        return (_lib.T2S_FILTER_TOP_K, k, 0.0)
    if name == "top_p":
        thres = float(kw.pop("thres", 0.9))
        if kw:
            raise ValueError(f"top_p takes thres, got {sorted(kw)}")
        if not 0.0 < thres < 1.0:
            raise ValueError(f"top_p: thres = {thres} outside (0, 1)")
        return (_lib.T2S_FILTER_TOP_P, 0, thres)
    raise ValueError(f"filter_logits_fn must be 'top_k' or 'top_p', got {filter_logits_fn!r}")


def sequence_logprob(logprobs: torch.Tensor, streams: torch.Tensor, eos: int) -> float:
    """The mean log-probability per counted token of one decoded utterance: per stream the positions up to AND INCLUDING its first eos
    count (all of them when it has none - what is behind an eos is padding, mask_after_eos, text2semantic.py:73-76); the result is the sum
    of logprobs over the counted positions of all streams divided by their number.  logprobs float [S, L], streams int64 [S, L] (what
    `generate(return_logprobs=True)` returns); summed in fp64 on the host."""
    lp, st = torch.as_tensor(logprobs).detach().cpu().double(), torch.as_tensor(streams).detach().cpu()
    if lp.shape != st.shape or lp.numel() == 0 or lp.ndim not in (1, 2):
        raise ValueError(f"sequence_logprob: logprobs {tuple(lp.shape)} and streams {tuple(st.shape)} must be the same non-empty [S, L]")
    lp, st = lp.reshape(-1, lp.shape[-1]), st.reshape(-1, st.shape[-1])
    counted = counted_mask(st, eos)
    return float(lp[counted].sum() / int(counted.sum()))


def counted_mask(streams: torch.Tensor, eos: int) -> torch.Tensor:
    """bool [S, L]: per stream the positions up to AND INCLUDING its first eos, all of them when it has none - the positions
    sequence_logprob counts and counted_tokens returns."""
    after = (streams == eos).cumsum(dim=-1) > 0
    return ~torch.nn.functional.pad(after, (1, -1), value=False)


def counted_tokens(streams, eos: int) -> list:
    """Per stream of `streams` (int64 [S, L] or [L]) its counted tokens as a 1-D host tensor: the positions up to and including the first
    eos, all positions when the stream has none (counted_mask: the set sequence_logprob averages over)."""
    st = torch.as_tensor(streams).detach().cpu()
    if st.ndim not in (1, 2) or st.dtype != torch.int64:
        raise ValueError(f"counted_tokens: streams {tuple(st.shape)} {st.dtype} must be int64 [S, L] or [L]")
    st = st.reshape(-1, st.shape[-1])
    mask = counted_mask(st, eos)
    return [row[m] for row, m in zip(st, mask)]


def consensus_pairs(n_candidates: int, streams: int) -> list:
    """The S N (N - 1) / 2 unordered pairs one utterance's risks are counted from, over its items in the order candidate-major,
    stream-minor (item c * S + s): (c, c', s) for c < c'."""
    return [(c * streams + s, c2 * streams + s) for c in range(n_candidates) for c2 in range(c + 1, n_candidates) for s in range(streams)]


def consensus_risks(candidates, eos: int):
    """Consensus (minimum-Bayes-risk) risks of the candidates of best-of-N: risk[c] = sum over the other candidates c' and the streams s
    of the edit distance between counted_tokens(c)[s] and counted_tokens(c')[s].  `candidates`: the (flat, streams[, logprobs]) tuples of
    ONE utterance -> list of N ints; or a LIST of such lists (utterances, which may differ in N) -> a list of lists, with the pairs of all
    utterances in ONE ops.edit_distance launch.  The distance is symmetric, so every unordered pair is computed once."""
    cands = list(candidates)
    one = bool(cands) and isinstance(cands[0], tuple)
    utts = [cands] if one else [list(u) for u in cands]
    seqs, pairs, spans = [], [], []
    for u in utts:
        if not u:
            raise ValueError("consensus_risks: an utterance without candidates")
        toks = [counted_tokens(c[1], eos) for c in u]
        S = len(toks[0])
        if any(len(t) != S for t in toks):
            raise ValueError("consensus_risks: the candidates of an utterance differ in their number of streams")
        base = len(seqs)
        seqs += [t for cand in toks for t in cand]
        here = consensus_pairs(len(u), S)
        spans.append((len(pairs), here, S))
        pairs += [(base + a, base + b) for a, b in here]
    dist = ops.edit_distance(seqs, pairs).tolist() if pairs else []
    out = []
    for u, (at, here, S) in zip(utts, spans):
        risk = [0] * len(u)
        for k, (a, b) in enumerate(here):
            risk[a // S] += dist[at + k]
            risk[b // S] += dist[at + k]
        out.append(risk)
    return out[0] if one else out


def consensus_candidate(risks, scores) -> int:
    """The index consensus selection keeps: the smallest risk; among equal risks the larger score under best_candidate's rule (a NaN
    never wins against a number); among those the lowest index."""
    risks, scores = [int(r) for r in risks], [float(x) for x in scores]
    if not risks or len(risks) != len(scores):
        raise ValueError(f"consensus_candidate: {len(risks)} risks and {len(scores)} scores")
    low = min(risks)
    tied = [c for c, r in enumerate(risks) if r == low]
    return tied[best_candidate([scores[c] for c in tied])]


def token_error_rate(pred, ref, pad: int = 501):
    """The reference's validation metric of text2semantic (covomix/util/inference.py:287-358: jiwer.wer over the token strings after both
    were padded with 501 to the longer length): edit distance(pred + pads, ref + pads) / padded length; two empty inputs give 0.0.
    pred, ref: 1-D int64 tensors -> float; or lists of them (equally long) -> a list of floats from ONE ops.edit_distance launch (the
    mean is the caller's)."""
    one = isinstance(pred, torch.Tensor)
    if one != isinstance(ref, torch.Tensor):
        raise ValueError("token_error_rate: one prediction and one reference, or a list of each")
    preds, refs = ([pred], [ref]) if one else (list(pred), list(ref))
    if len(preds) != len(refs):
        raise ValueError(f"token_error_rate: {len(preds)} predictions and {len(refs)} references")
    seqs, lens = [], []
    for p_, r_ in zip(preds, refs):
        p_, r_ = (torch.as_tensor(x).detach().cpu().reshape(-1).to(torch.int64) for x in (p_, r_))
        L = max(p_.numel(), r_.numel())
        seqs += [torch.nn.functional.pad(x, (0, L - x.numel()), value=pad) for x in (p_, r_)]
        lens.append(L)
    live = [k for k, L in enumerate(lens) if L > 0]
    dist = ops.edit_distance(seqs, [(2 * k, 2 * k + 1) for k in live]).tolist() if live else []
    out = [0.0] * len(lens)
    for k, d in zip(live, dist):
        out[k] = d / lens[k]
    return out[0] if one else out


def best_candidate(scores) -> int:
    """best-of-N: the index of the largest score; the LOWEST index wins ties.  A NaN score never wins against a number."""
    scores = [float(x) for x in scores]
    if not scores:
        raise ValueError("best_candidate: no candidates")
    best = 0
    for c in range(1, len(scores)):
        if scores[c] > scores[best] or (math.isnan(scores[best]) and not math.isnan(scores[c])):
            best = c
    return best


def check_best_of(best_of, n_utterances: Optional[int] = None, uniforms=None) -> int:
    """best_of of synthesis_sample_text2semantic: an integer >= 1; caller-supplied uniforms then hold the draws of every candidate,
    [best_of, steps, S, V] per utterance.  ValueError otherwise."""
    if isinstance(best_of, bool) or not isinstance(best_of, int) or best_of < 1:
        raise ValueError(f"best_of must be an integer >= 1, got {best_of!r}")
    if best_of > 1 and uniforms is not None:
        us = [uniforms] if n_utterances is None else list(uniforms)
        if n_utterances is not None and len(us) != n_utterances:
            raise ValueError(f"best_of: {len(us)} uniform tensors for {n_utterances} utterances")
        for u in us:
            if u.ndim < 4 or u.shape[0] != best_of:
                raise ValueError(f"best_of = {best_of}: the uniforms of an utterance are [best_of, steps, S, V], got {tuple(u.shape)}")
    return best_of


def check_beam_size(beam_size) -> int:
    """beam_size of generate_beam: an integer in [1, BEAM_MAX].  ValueError otherwise."""
    if isinstance(beam_size, bool) or not isinstance(beam_size, int) or not 1 <= beam_size <= BEAM_MAX:
        raise ValueError(f"beam_size must be an integer in [1, {BEAM_MAX}], got {beam_size!r}")
    return beam_size


def check_beam_scale(cond_scale) -> float:
    """the guidance scale of a beam search: 1 (unguided) or > 1 (guided)"""
    scale = float(cond_scale)
    if not scale >= 1.0:
        raise ValueError(f"beam search: cond_scale = {cond_scale} must be >= 1")
    return scale


def beam_backtrack(parents, tokens, logprobs, slot: int, steps: int):
    """The sequence of the hypothesis that sits in `slot` after `steps` steps, from the back-pointer records of the selection step:
    parents [T, B] (the slot the hypothesis came from), tokens [T, B, S], logprobs [T, B, S] -> (tokens [S, steps], logprobs [S, steps],
    path [steps]: the slot at every step).  What the device's back-track kernel computes."""
    S = tokens.shape[2]
    tk = torch.zeros(S, steps, dtype=tokens.dtype)
    lp = torch.zeros(S, steps, dtype=logprobs.dtype)
    path = [0] * steps
    cur = int(slot)
    for t in range(steps - 1, -1, -1):
        path[t] = cur
        tk[:, t], lp[:, t] = tokens[t, cur], logprobs[t, cur]
        cur = int(parents[t, cur])
    return tk, lp, path


def beam_rank(scores, lengths, streams: int, length_penalty: float = 1.0) -> list:
    """Slots of one utterance, best first: by c / n ** length_penalty with c the cumulative log-probability and n = steps * streams the
    tokens scored (up to and including the eos step); ties - and dead hypotheses, c = -inf, last - go to the lowest slot."""
    def value(i):
        n = int(lengths[i]) * streams
        c = float(scores[i])
        return c / float(n) ** float(length_penalty) if n > 0 and c > -math.inf else -math.inf
    vals = [value(i) for i in range(len(scores))]
    return sorted(range(len(vals)), key=lambda i: (-vals[i], i))


def check_targets(targets, streams: int, vocab: int, max_length: int) -> list:
    """The targets of score_many as int64 [S, L] host tensors.  ValueError for a shape other than [S, L] ([L] is taken as [1, L]),
    L < 1, L > max_length or a token outside [0, vocab): such a token must never reach the device, where it would index the embedding."""
    out = []
    for j, t in enumerate(targets):
        t = torch.as_tensor(t).detach().cpu()
        if t.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"target {j}: integer tokens expected, got {t.dtype}")
        t = t.to(torch.int64)
        if t.ndim == 1:
            t = t[None, :]
        if t.ndim != 2 or t.shape[0] != streams:
            raise ValueError(f"target {j}: [S = {streams}, L] expected, got {tuple(t.shape)}")
        L = t.shape[1]
        if L < 1 or L > max_length:
            raise ValueError(f"target {j}: length {L} outside [1, max_length = {max_length}]")
        if int(t.min()) < 0 or int(t.max()) >= vocab:
            raise ValueError(f"target {j}: tokens outside [0, vocab = {vocab})")
        out.append(t.contiguous())
    return out


class UtteranceSettings(NamedTuple):
    """Sampling settings of ONE utterance of generate_many(settings=...): every field left None takes the call's scalar argument."""
    temperature: Optional[float] = None
    filter_logits_fn: Optional[object] = None
    filter_fn_kwargs: Optional[dict] = None
    cond_scale: Optional[float] = None
    repetition_penalty: Optional[float] = None
    repetition_window: Optional[int] = None
    no_repeat_ngram_size: Optional[int] = None
    min_length: Optional[int] = None


SETTING_FIELDS = UtteranceSettings._fields
RULE_FIELDS = ("repetition_penalty", "repetition_window", "no_repeat_ngram_size", "min_length")      # the history rules (check_rules)
RULES_OFF = (1.0, 0, 0, 0)


def _setting_entry(e) -> dict:
    """one entry of `settings` (None, a mapping, a record) as a dict"""
    if e is None:
        return {}
    if isinstance(e, Mapping):
        return dict(e)
    if hasattr(e, "_asdict"):
        return e._asdict()
    return {f: getattr(e, f) for f in SETTING_FIELDS if hasattr(e, f)}


def check_settings(settings, n: int, vocab: int, streams: int = 1, temperature: float = 1.0, filter_logits_fn="top_k", filter_fn_kwargs=None,
                   cond_scale: float = 1.0, mixed: bool = False) -> list:
    """The per-utterance settings of generate_many resolved against the call's scalars: -> n tuples (temperature, (mode, k, thres),
    cond_scale).  settings: n entries, each None (the scalars apply), a mapping or a record with any of the fields of UtteranceSettings
    (an absent or None field takes the scalar; a filter_logits_fn without filter_fn_kwargs takes that filter's defaults, not the call's
    kwargs of another filter).  ValueError for another length, an unknown field, a temperature < 0 (or NaN), whatever `filter_setting`
    refuses, a cond_scale <= 1 in a guided call (the call's cond_scale > 1) and a cond_scale other than 1 in an unguided call: the slot-pair
    layout of guidance belongs to the launch, so guided and unguided utterances do not share one - make two calls.  NotImplementedError for
    guidance on a two-output model, as everywhere.  Pure host code.
    mixed (generate_many(mixed_guidance=True): the pair layout belongs to the dialogue record there): the call's cond_scale is only the
    default, and every utterance may have a scale of exactly 1 (unguided) or > 1 (guided); any other value (< 1, NaN) is a ValueError,
    and any scale > 1 on a two-output model a NotImplementedError."""
    settings = list(settings)
    if len(settings) != n:
        raise ValueError(f"settings: {len(settings)} entries for {n} utterances")
    guided = float(cond_scale) > 1.0
    if guided and streams != 1 and not mixed:
        raise NotImplementedError("guidance (cond_scale > 1) on a two-output model: the reference cannot run it (generate_batch)")
    out = []
    for j, e in enumerate(settings):
        e = _setting_entry(e)
        unknown = sorted(set(e) - set(SETTING_FIELDS))
        if unknown:
            raise ValueError(f"settings[{j}]: unknown fields {unknown}; known: {list(SETTING_FIELDS)}")
        t = float(temperature if e.get("temperature") is None else e["temperature"])
        if not t >= 0.0:
            raise ValueError(f"settings[{j}]: temperature = {t} must be >= 0")
        if e.get("filter_logits_fn") is not None:
            fn, kw = e["filter_logits_fn"], e.get("filter_fn_kwargs")
        else:
            fn, kw = filter_logits_fn, (filter_fn_kwargs if e.get("filter_fn_kwargs") is None else e["filter_fn_kwargs"])
        try:
            filt = filter_setting(fn, kw, vocab)
        except ValueError as err:
            raise ValueError(f"settings[{j}]: {err}") from None
        c = float(cond_scale if e.get("cond_scale") is None else e["cond_scale"])
        if mixed:
            if not c >= 1.0:
                raise ValueError(f"settings[{j}]: cond_scale = {c}: an utterance is unguided (exactly 1) or guided (> 1)")
            if c > 1.0 and streams != 1:
                raise NotImplementedError("guidance (cond_scale > 1) on a two-output model: the reference cannot run it (generate_batch)")
            out.append((t, filt, c))
            continue
        if guided and not c > 1.0:
            raise ValueError(f"settings[{j}]: cond_scale = {c} in a guided call (cond_scale > 1): guided and unguided utterances do not share "
                             "a launch - make two calls")
        if not guided and c != 1.0:
            if c > 1.0 and streams != 1:
                raise NotImplementedError("guidance (cond_scale > 1) on a two-output model: the reference cannot run it (generate_batch)")
            raise ValueError(f"settings[{j}]: cond_scale = {c} in an unguided call (cond_scale = 1): guided and unguided utterances do not "
                             "share a launch - make two calls")
        out.append((t, filt, c))
    return out


def settings_rows(resolved, prefix_lens=None) -> torch.Tensor:
    """The rows of the device's settings table (cvx_t2s_per_dialogue; include/covomix_hip.h) for the tuples of check_settings: int32
    [n, 8] holding [0] inv_temp = 1 / max(temperature, 1e-10) computed in fp32 - the bits cvx_t2s_decode_steps computes - [1] filter mode
    [2] top_k [3] top_p [4] cond_scale (fp32 bits) [5] prefix length (default 0) [6], [7] 0."""
    n = len(resolved)
    rows = torch.zeros(n, _lib.T2S_PER_WORDS, dtype=torch.int32)
    if n == 0:
        return rows
    f = lambda xs: torch.tensor(xs, dtype=torch.float64).to(torch.float32)       # (python floats round to fp32 as ctypes' c_float does)
    inv = torch.ones(n, dtype=torch.float32) / torch.maximum(f([r[0] for r in resolved]), torch.tensor(1e-10, dtype=torch.float32))
    rows[:, 0] = inv.view(torch.int32)
    rows[:, 1] = torch.tensor([r[1][0] for r in resolved], dtype=torch.int32)
    rows[:, 2] = torch.tensor([r[1][1] for r in resolved], dtype=torch.int32)
    rows[:, 3] = f([r[1][2] for r in resolved]).view(torch.int32)
    rows[:, 4] = f([r[2] for r in resolved]).view(torch.int32)
    if prefix_lens is not None:
        rows[:, 5] = torch.tensor([int(x) for x in prefix_lens], dtype=torch.int32)
    return rows


def check_rules(settings, n: int, max_length: int, repetition_penalty: float = 1.0, repetition_window: int = 0,
                no_repeat_ngram_size: int = 0, min_length: int = 0) -> list:
    """The history rules of n utterances resolved against the call's scalars: -> n tuples (theta, W, ngram, min_len) - the repetition
    penalty theta > 0 (1: off) over the last W >= 0 tokens of a stream (0: all of them), the no-repeat n-gram size in 0..8 (0: off) and
    the minimum length (the eos is not selectable below it); the definition: include/covomix_hip.h, cvx_t2s_decode_steps_rules.
    settings: None (the scalars for everyone) or n entries as `check_settings` takes them; a field an entry leaves out or None takes the
    scalar, other fields are not looked at.  ValueError: another length, a penalty that is not a finite number > 0, W < 0, an n-gram size
    outside 0..8, a minimum length < 0 or > max_length, a non-integer W / size / length.  Pure host code."""
    entries = [None] * n if settings is None else list(settings)
    if len(entries) != n:
        raise ValueError(f"settings: {len(entries)} entries for {n} utterances")
    scalars = dict(zip(RULE_FIELDS, (repetition_penalty, repetition_window, no_repeat_ngram_size, min_length)))

    def whole(name, v, where):
        if isinstance(v, bool) or (not isinstance(v, int) and not (isinstance(v, float) and v == int(v))):
            raise ValueError(f"{where}{name} = {v!r} must be an integer")
        return int(v)
    out = []
    for j, e in enumerate([None] + entries):               # (the scalars themselves first: a bad scalar is refused whatever the entries say)
        e = _setting_entry(e)
        where = "" if j == 0 else f"settings[{j - 1}]: "
        get = lambda f: scalars[f] if e.get(f) is None else e[f]
        try:
            theta = float(get("repetition_penalty"))
        except (TypeError, ValueError):
            raise ValueError(f"{where}repetition_penalty = {get('repetition_penalty')!r} must be a number") from None
        if not (theta > 0.0 and math.isfinite(theta)):
            raise ValueError(f"{where}repetition_penalty = {theta} must be a finite number > 0 (1 is off)")
        W = whole("repetition_window", get("repetition_window"), where)
        if W < 0:
            raise ValueError(f"{where}repetition_window = {W} must be >= 0 (0: the whole history)")
        ng = whole("no_repeat_ngram_size", get("no_repeat_ngram_size"), where)
        if not 0 <= ng <= _lib.T2S_RULES_MAX_NGRAM:
            raise ValueError(f"{where}no_repeat_ngram_size = {ng} outside 0..{_lib.T2S_RULES_MAX_NGRAM} (0 is off)")
        m = whole("min_length", get("min_length"), where)
        if not 0 <= m <= int(max_length):
            raise ValueError(f"{where}min_length = {m} outside [0, max_length = {int(max_length)}]")
        if j:
            out.append((theta, W, ng, m))
    return out


def rules_active(resolved) -> bool:
    """does any tuple of check_rules switch a rule on?  (A penalty of 1 with any window, n-gram size 0 and minimum length 0 change nothing.)"""
    return any(r[0] != 1.0 or r[2] != 0 or r[3] != 0 for r in resolved)


def rules_rows(resolved) -> torch.Tensor:
    """The rows of the device's rules table (cvx_t2s_rules; include/covomix_hip.h) for the tuples of check_rules: int32 [n, 4] holding
    [0] theta (fp32 bits) [1] window [2] n-gram size [3] minimum length."""
    n = len(resolved)
    rows = torch.zeros(n, _lib.T2S_RULES_WORDS, dtype=torch.int32)
    if n == 0:
        return rows
    rows[:, 0] = torch.tensor([r[0] for r in resolved], dtype=torch.float64).to(torch.float32).view(torch.int32)
    for c in (1, 2, 3):
        rows[:, c] = torch.tensor([int(r[c]) for r in resolved], dtype=torch.int32)
    return rows


def check_beam_rules(n: int, max_length: int, repetition_penalty=1.0, repetition_window=0, no_repeat_ngram_size=0, min_length=0) -> list:
    """The history rules of n utterances of a beam search under `beam_rules` (the definition: include/covomix_hip.h,
    cvx_t2s_beam_rules_steps): no_repeat_ngram_size and min_length, each a scalar or one value per utterance, validated by `check_rules`
    -> n tuples (1.0, 0, ngram, min_len) for `rules_rows`.  ValueError: what check_rules refuses, a list of another length than n, and a
    repetition penalty other than 1 - it would make the search score something other than the model's log-probability - or a repetition
    window other than 0, the window of a penalty there is none of.  Pure host code."""
    per = {}
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_length", min_length)):
        if isinstance(v, (list, tuple)) or torch.is_tensor(v):
            vals = v.tolist() if torch.is_tensor(v) else list(v)
            if len(vals) != n:
                raise ValueError(f"beam search: {len(vals)} values of {name} for {n} utterances")
            per[name] = vals
    scalar = lambda name, v: 0 if name in per else v
    settings = [{k: vals[j] for k, vals in per.items()} for j in range(n)] if per else None
    resolved = check_rules(settings, n, max_length, repetition_penalty, repetition_window, scalar("no_repeat_ngram_size", no_repeat_ngram_size),
                           scalar("min_length", min_length))
    if any(r[0] != 1.0 for r in resolved):
        raise ValueError("beam search takes no repetition_penalty: a penalty would make the search score something other than the model's "
                         "log-probability - leave it at 1 (no_repeat_ngram_size and min_length run under beam_rules)")
    if any(r[1] != 0 for r in resolved):
        raise ValueError("beam search takes no repetition_window: it is the window of the repetition penalty, which beam search does not run")
    return [(1.0, 0, r[2], r[3]) for r in resolved]


def mixed_records(kinds) -> list:
    """The dialogue record of every utterance of a mixed call (cvx_t2s_decode_steps_mixed): a guided utterance (kinds[j] true) takes two
    records - its text half, which is the one returned, and the null half behind it - an unguided one takes one.  -> n + 1 numbers, the
    last one the number of records."""
    first, r = [], 0
    for g in kinds:
        first.append(r)
        r += 2 if g else 1
    return first + [r]


def mixed_windows(kinds, window: int = WINDOW) -> list:
    """Utterance ranges [(begin, end), ...] of a mixed call cut so that every range holds at most `window` dialogue RECORDS and no
    guided pair is cut: a range ends where the next utterance would not fit whole."""
    out, begin, used = [], 0, 0
    for j, g in enumerate(kinds):
        need = 2 if g else 1
        if used + need > window:
            out.append((begin, j))
            begin, used = j, 0
        used += need
    if begin < len(kinds):
        out.append((begin, len(kinds)))
    return out


def mixed_schedule(kinds, lengths, slots: int, n_records: Optional[int] = None) -> list:
    """The device's scheduler (mixed_schedule_kernel; include/covomix_hip.h, cvx_t2s_decode_steps_mixed) replayed on the host, given the
    number of steps every utterance takes: -> per utterance (slot, null slot or None, start step), or None for an utterance that is
    never taken.  kinds[j]: utterance j is guided; lengths[j] >= 1: its steps; slots: the decode slots.  The policy: after every step
    (and once before the first: start step 0) the idle slots F in ascending order serve the queue head - an unguided record takes the
    lowest slot of F; a guided one takes the two lowest (text half, null half) and WAITS, with everything behind it, while F holds fewer
    than two.  An utterance that starts at step s with L steps frees its slot(s) for the scheduler run after step s + L.
    n_records (default: all): the queue's record count - a guided head whose second record lies beyond it is never taken, nor is
    anything behind it.  For tests and tools; the decode does not call it."""
    n = len(kinds)
    if len(lengths) != n or slots < 1 or any(int(x) < 1 for x in lengths):
        raise ValueError("mixed_schedule: one length >= 1 per utterance and at least one slot")
    first = mixed_records(kinds)
    total = first[-1] if n_records is None else int(n_records)
    out: list = [None] * n
    free = list(range(int(slots)))
    busy: list = []                        # (step at which the slots idle, slots)
    h, t = 0, 0
    while True:
        while h < n and free and first[h] < total:
            if not kinds[h]:
                s0 = free.pop(0)
                out[h] = (s0, None, t)
                busy.append((t + int(lengths[h]), [s0]))
            else:
                if first[h] + 1 >= total or len(free) < 2:
                    break
                s0, s1 = free.pop(0), free.pop(0)
                out[h] = (s0, s1, t)
                busy.append((t + int(lengths[h]), [s0, s1]))
            h += 1
        if not busy:
            break
        t = min(e for e, _ in busy)
        for e, ss in busy:
            if e == t:
                free += ss
        busy = [x for x in busy if x[0] != t]
        free.sort()
    return out


def check_prefixes(prefixes, n: int, streams: int, vocab: int, limits, forced=None) -> list:
    """The prefixes of generate_many as int64 [S, P] host tensors (None: no prefix).  ValueError for another number of entries, whatever
    `check_targets` refuses (shape, P < 1, a token outside [0, vocab)), P >= that utterance's step limit (nothing would be left to decode),
    an eos inside a prefix (continuing past an end is not defined by the reference loop) and a prefix for an utterance that is forced."""
    prefixes = list(prefixes)
    if len(prefixes) != n:
        raise ValueError(f"prefixes: {len(prefixes)} entries for {n} utterances")
    out: list = [None] * n
    for j, p in enumerate(prefixes):
        if p is None:
            continue
        if forced is not None and forced[j] is not None:
            raise ValueError(f"prefix {j}: the utterance is forced - its tokens are all given already")
        try:
            t = check_targets([p], streams, vocab, max(int(limits[j]), 1))[0]
        except ValueError as err:
            raise ValueError(f"prefix {j}: {err}") from None
        if t.shape[1] >= int(limits[j]):
            raise ValueError(f"prefix {j}: length {t.shape[1]} leaves nothing to decode below the step limit {int(limits[j])}")
        if bool((t == vocab - 1).any()):
            raise ValueError(f"prefix {j}: holds an eos (token {vocab - 1}); continuing past an end is not defined")
        out[j] = t
    return out


PREFILL_ROWS = 32768           # packed rows of one prefill pass (its buffers: [M, 3 inner], [M, 2 ff], [M, S, V])


def prefill_rows(seqs, streams: int, max_length: int, ctx_rows: int) -> dict:
    """The packed tables of ONE prefill pass (TextToSemanticDecoder._prefill; the definition: include/covomix_hip.h,
    cvx_t2s_prefill_attention_f32).  seqs: one entry per sequence, (tokens int64 [S, L], record, ctx, slot): the L >= 1 given tokens
    (sequence i then has L input rows at positions 0 .. L - 1: row 0 is the start token, row p > 0 the embeddings of tokens[:, p - 1]),
    the dialogue record whose kv_c rows [0, ctx) its cross-attention reads (ctx = 1: the null half of a guided pair) and the decode slot
    whose caches take its rotated keys and values - None for all sequences or for none.  -> host tensors:
      cu int32 [n + 1]       packed rows per sequence            positions int64 [M]   position of every row (the RoPE rows)
      gather int64 [M, S]    embedding row per (row, stream); 0 on a sequence's first row, which `starts` int64 [n] names
      targets int64 [M, S]   tokens[:, p]: the token row p's logits are scored at
      kbase, nk int32 [n]    first kv_c row (record * ctx_rows) and key count (ctx) of the cross-attention
      cache int64 [M]        flat cache row slot * max_length + position (None without slots)
    and rows = M, max_q = the longest sequence.  ValueError: no sequence, a shape other than [S, L], L outside [1, max_length], ctx
    outside [1, ctx_rows], a negative record or slot, slots for some sequences only.  Pure host code."""
    seqs = list(seqs)
    if not seqs:
        raise ValueError("prefill_rows: no sequence")
    cu, pos, gather, targets, kbase, nk, cache = [0], [], [], [], [], [], []
    with_slots = seqs[0][3] is not None
    for i, (tok, record, ctx, slot) in enumerate(seqs):
        tok = torch.as_tensor(tok).detach().cpu().to(torch.int64)
        if tok.ndim != 2 or tok.shape[0] != streams or not 1 <= tok.shape[1] <= max_length:
            raise ValueError(f"prefill_rows: sequence {i}: [S = {streams}, 1 <= L <= {max_length}] tokens expected, got {tuple(tok.shape)}")
        if not 1 <= int(ctx) <= ctx_rows or int(record) < 0:
            raise ValueError(f"prefill_rows: sequence {i}: record {record} with {ctx} context rows (1..{ctx_rows})")
        if (slot is not None) != with_slots or (with_slots and int(slot) < 0):
            raise ValueError("prefill_rows: a decode slot for every sequence or for none")
        L = tok.shape[1]
        p = torch.arange(L, dtype=torch.int64)
        cu.append(cu[-1] + L)
        pos.append(p)
        gather.append(torch.cat((torch.zeros(1, streams, dtype=torch.int64), tok[:, :L - 1].T), dim=0))
        targets.append(tok.T)
        kbase.append(int(record) * ctx_rows)
        nk.append(int(ctx))
        if with_slots:
            cache.append(p + int(slot) * max_length)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32)
    return dict(cu=i32(cu), positions=torch.cat(pos), gather=torch.cat(gather).contiguous(), starts=torch.tensor(cu[:-1], dtype=torch.int64),
                targets=torch.cat(targets).contiguous(), kbase=i32(kbase), nk=i32(nk), cache=torch.cat(cache) if with_slots else None,
                rows=cu[-1], max_q=max(b - a for a, b in zip(cu, cu[1:])))


def prefill_windows(rows, cap: int = PREFILL_ROWS, records=None, window: int = WINDOW) -> list:
    """Utterance ranges [(begin, end), ...] of the prefill passes of a call: rows[j] = the packed rows utterance j brings (both halves of a
    guided one), at most `cap` per pass - and, with records[j] = its dialogue records, at most `window` of those.  An utterance is never
    cut: a range ends where the next one would not fit whole, and one that exceeds the cap alone is a pass of its own."""
    out, begin, used, recs = [], 0, 0, 0
    for j, r in enumerate(rows):
        need = 0 if records is None else int(records[j])
        if j > begin and (used + int(r) > cap or recs + need > window):
            out.append((begin, j))
            begin, used, recs = j, 0, 0
        used += int(r)
        recs += need
    if begin < len(rows):
        out.append((begin, len(rows)))
    return out


def _dims(sd: Dict[str, torch.Tensor]) -> dict:
    dim = sd["token_emb.text.weight"].shape[1]
    dim_t = sd["start_token.speech"].shape[0]
    emb = sd["semantic_token_emb.weight"].shape[1]
    heads = sd["target_transformer.layers.0.1.null_kv"].shape[1]
    if sd["target_transformer.layers.0.1.null_kv"].shape[-1] != 64:
        raise ValueError("only dim_head == 64 is supported (reference default)")
    if emb not in (dim_t, dim_t // 2):
        raise ValueError("semantic embedding width must be the target width (one output) or half of it (two outputs)")
    depth = lambda pre: len({k.split(".")[2] for k in sd if k.startswith(pre + ".layers.")})
    ff = lambda pre: sd[pre + ".layers.0.2.4.weight"].shape[1]
    return dict(dim=dim, dim_target=dim_t, dim_emb=emb, streams=dim_t // emb, heads=heads, inner=heads * 64,
                source_depth=depth("source_transformer"), target_depth=depth("target_transformer"),
                vocab=sd["semantic_token_emb.weight"].shape[0], ff_src=ff("source_transformer"), ff_tgt=ff("target_transformer"),
                text_eos=sd["token_emb.text.weight"].shape[0] - 1)


def _half_split_rows(w: torch.Tensor, heads: int) -> torch.Tensor:
    """Rows of a [heads*64, K] projection reordered (0,2,..,62,1,3,..,63) inside every head."""
    perm = torch.cat((torch.arange(0, 64, 2), torch.arange(1, 64, 2))).to(w.device)
    return w.reshape(heads, 64, -1)[:, perm, :].reshape(heads * 64, -1).contiguous()


def _pad_cols(w: torch.Tensor, mult: int = 4) -> torch.Tensor:
    k = w.shape[1]
    kp = (k + mult - 1) // mult * mult
    if kp == k:
        return w.contiguous()
    out = torch.zeros(w.shape[0], kp, dtype=w.dtype, device=w.device)
    out[:, :k] = w
    return out


class TextToSemanticDecoder:
    """Device-resident packed weights of one TextToSemantic network + encode / generate."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device: torch.device, max_length: int = 2048, max_source: int = 1024):
        sd = {k: v.detach().to(device=device, dtype=torch.float32).contiguous() for k, v in state_dict.items()}
        self.device = device
        self.d = d = _dims(sd)
        self.max_length, self.max_source = int(max_length), int(max_source)
        H, I = d["heads"], d["inner"]
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)

        def attn_pack(p, self_attn):
            wq, wkv = sd[p + ".to_q.0.weight"], sd[p + ".to_kv.0.weight"]
            wk, wv = wkv[:I], wkv[I:]
            if self_attn:
                return torch.cat((_half_split_rows(wq, H), _half_split_rows(wk, H), wv), dim=0).contiguous()
            return wq.contiguous(), wkv.contiguous()

        self.emb_text = sd["token_emb.text.weight"]
        self.emb = sd["semantic_token_emb.weight"]
        self.start = sd["start_token.speech"]
        # ---- encoder
        self.enc = []
        for i in range(d["source_depth"]):
            p = f"source_transformer.layers.{i}"
            self.enc.append(dict(gamma_a=sd[p + ".0.norm.gamma"], wqkv=attn_pack(p + ".0", True), wo=sd[p + ".0.to_out.weight"],
                                 gamma_f=sd[p + ".2.0.gamma"], w1=sd[p + ".2.1.weight"], b1=sd[p + ".2.1.bias"],
                                 w2=_pad_cols(sd[p + ".2.4.weight"]), b2=sd[p + ".2.4.bias"]))
        self.enc_final = sd["source_transformer.final_norm.gamma"]
        self.freqs_src = sd["source_transformer.layers.0.0.rotary_emb.freqs"]
        # ---- decoder
        self.Fp = (d["ff_tgt"] + 3) // 4 * 4
        self.dec = []
        for i in range(d["target_depth"]):
            p = f"target_transformer.layers.{i}"
            wq_c, wkv_c = attn_pack(p + ".1", False)
            nkv = sd[p + ".1.null_kv"]                                    # [2, H, 1, 64]
            self.dec.append(dict(gamma_s=sd[p + ".0.norm.gamma"], wqkv_s=attn_pack(p + ".0", True), wo_s=sd[p + ".0.to_out.weight"],
                                 gamma_c=sd[p + ".1.norm.gamma"], wq_c=wq_c, wkv_c=wkv_c, wo_c=sd[p + ".1.to_out.weight"],
                                 null=torch.cat((nkv[0].reshape(I), nkv[1].reshape(I))).contiguous(),
                                 gamma_f=sd[p + ".2.0.gamma"], w1=sd[p + ".2.1.weight"], b1=sd[p + ".2.1.bias"],
                                 w2=_pad_cols(sd[p + ".2.4.weight"]), b2=sd[p + ".2.4.bias"]))
        self.dec_final = sd["target_transformer.final_norm.gamma"]
        pos = torch.arange(self.max_length, device=device, dtype=torch.float32)
        ang = pos[:, None] * sd["target_transformer.layers.0.0.rotary_emb.freqs"][None, :]
        self.rope = (ang.cos().contiguous(), ang.sin().contiguous())
        self.top_k = math.ceil(TOP_K_THRES * d["vocab"])
        self._default_filter = filter_setting(vocab=d["vocab"])         # (top_k, k = ceil(0.1 V)): the reference's default
        self.buf: Dict[str, torch.Tensor] = {}
        self._slots = self._dialogues = self._steps = 0   # capacities of the decode buffers (_ensure)
        self._gen = 0                                      # bumped when they are re-allocated (captured graphs hold their addresses)
        self._layers = (_lib.T2SLayer * d["target_depth"])()
        for i, L in enumerate(self.dec):
            for name in ("gamma_s", "wqkv_s", "wo_s", "gamma_c", "wq_c", "wo_c", "gamma_f", "w1", "b1", "w2", "b2"):
                setattr(self._layers[i], name, L[name].data_ptr())
        self._graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self._cap = None                                   # capture stream of the decode graphs
        self._stage = None                                 # staging copies of the state record (two in flight), _chunks
        self._ensure(8, 8, 0)

    @staticmethod
    def _slot_capacity(n: int) -> int:
        """per-slot buffers hold whole kernel groups: 1 / 2 / 4 slots, or a multiple of 8 (include/covomix_hip.h)"""
        return n if n in (1, 2, 4) else (n + 7) // 8 * 8

    def _ensure(self, slots: int, dialogues: int, steps: int, logprobs: bool = False) -> None:
        """Decode buffers for `slots` decode slots (x, q, att, h, logits, slot records, the self-attention caches), `dialogues`
        utterances in flight or queued (context k/v, token rows, dialogue records) and `steps` uniform draws per dialogue.  They only
        grow; growing re-allocates (and drops the captured graphs, which hold the old addresses).  The uniform draws per dialogue
        are rounded up to whole chunks of CHUNK steps: a lock-step decode (_chunks) runs whole chunks, and its sampling kernel
        reads the draws of every position it reaches (up to the model's max_length, whatever the call's max_length).
        logprobs: the log-prob buffer [dialogues, streams, max_length] of the scored decode as well - allocated on first use only (only
        scored graphs hold its address, so allocating it leaves the captured graphs alone), and re-allocated with the token rows."""
        d, dev = self.d, self.device
        S, V, I = d["streams"], d["vocab"], d["inner"]
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        slots = max(8, self._slot_capacity(slots))
        grown = False
        if slots > self._slots:
            self.buf.update(x=f32(slots, d["dim_target"]), q=f32(slots, I), att=f32(slots, I), h=f32(slots, self.Fp), logits=f32(slots, S, V),
                            state=torch.zeros(slots, SR, dtype=torch.int32, device=dev))
            for i, L in enumerate(self.dec):
                L["k_cache"], L["v_cache"] = f32(slots, self.max_length, I), f32(slots, self.max_length, I)
                self._layers[i].k_cache, self._layers[i].v_cache = L["k_cache"].data_ptr(), L["v_cache"].data_ptr()
            self._slots, grown = slots, True
        if dialogues > self._dialogues:
            dialogues = max(dialogues, 8)
            for i, L in enumerate(self.dec):
                L["kv_c"] = f32(dialogues, self.max_source + 2, 2 * I)
                self._layers[i].kv_c = L["kv_c"].data_ptr()
            self.buf.update(tokens=torch.zeros(dialogues, S, self.max_length, dtype=torch.int64, device=dev),
                            dialogues=torch.zeros(dialogues, SR, dtype=torch.int32, device=dev),
                            queue=torch.zeros(2, dtype=torch.int32, device=dev),
                            per=torch.zeros(dialogues, _lib.T2S_PER_WORDS, dtype=torch.int32, device=dev),
                            rules=torch.zeros(dialogues, _lib.T2S_RULES_WORDS, dtype=torch.int32, device=dev))
            self.buf.pop("logprobs", None)
            self._dialogues, grown = dialogues, True
        if logprobs and "logprobs" not in self.buf:
            self.buf["logprobs"] = f32(self._dialogues, S, self.max_length)
        steps = (max(steps, 1) + CHUNK - 1) // CHUNK * CHUNK
        if steps > self._steps or "uniforms" not in self.buf or self.buf["uniforms"].numel() < self._dialogues * self._steps * S * V:
            self._steps = max(self._steps, steps)
            self.buf["uniforms"] = f32(self._dialogues * self._steps * S * V)
            grown = True
        if grown:
            self._graphs.clear()
            self._stage = None
            self._gen += 1

    # ------------------------------------------------------------------ encoder (text2semantic.py:716-741)
    def _source_rows(self, source_ids: torch.Tensor) -> torch.Tensor:
        if source_ids.ndim == 2 and source_ids.shape[0] != 1:
            raise NotImplementedError("one utterance per entry (the generation scripts run batch 1)")
        ids = source_ids.reshape(-1).to(torch.int64)
        if bool((ids == 0).any()):
            raise NotImplementedError("padded text batches (id 0) are not supported: one un-padded utterance per call")
        if ids.numel() + 1 > self.max_source:
            raise ValueError(f"text of {ids.numel()} tokens exceeds max_source = {self.max_source}")
        return torch.cat((ids.cpu(), torch.tensor([self.d["text_eos"]])))                    # set_eos_id, no padding

    def encode_many(self, sources):
        """The source transformer over SEVERAL texts as one packed batch (rows of text i: [cu[i], cu[i + 1]); attention and rotary
        positions per text): the reference encodes one utterance per call, and a 65-token text alone is 19 GEMM launches of 30 us
        each on a handful of CUs - 64 dialogues encoded one by one cost a quarter of their decode.  Row results do not depend on the
        other rows of the batch.  -> (encoder output [M, dim], ops.Ragged)"""
        d = self.d
        rows = [self._source_rows(s_) for s_ in sources]
        rg = ops.Ragged([r.numel() for r in rows], self.device)
        src = ops.h2d(torch.cat(rows), self.device)
        M, H, I, D = rg.M, d["heads"], d["inner"], d["dim"]
        x = self.emb_text.index_select(0, src).contiguous()
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)
        normed, qkv, att = f(M, D), f(M, 3 * I), f(M, I)
        F_ = d["ff_src"]
        Fp = (F_ + 3) // 4 * 4
        h2, hg = f(M, 2 * F_), f(M, Fp)
        ang = rg.positions()[:, None] * self.freqs_src[None, :]
        rope = (ang.cos().contiguous(), ang.sin().contiguous())          # per-row tables (rope_T = M)
        for L in self.enc:
            ops.adarmsnorm(x, L["gamma_a"], None, normed)
            ops.gemm(normed, L["wqkv"], qkv, rope=rope, rope_cols=2 * I)
            ops.attention(qkv, att, 1, M, H, 64 ** -0.5, ragged=rg)
            ops.gemm(att, L["wo"], x, residual=x)
            ops.adarmsnorm(x, L["gamma_f"], None, normed)
            ops.gemm(normed, L["w1"], h2, bias=L["b1"])
            ops.geglu(h2, hg, F_)
            ops.gemm(hg, L["w2"], x, bias=L["b2"], residual=x)
        enc = f(M, D)
        ops.adarmsnorm(x, self.enc_final, None, enc)
        return enc, rg

    def encode(self, source_ids: torch.Tensor) -> torch.Tensor:
        return self.encode_many([source_ids])[0]

    # ------------------------------------------------------------------ decoder
    def _descriptor(self, temperature: float, batch: int = 1, cfg_scale: float = 1.0, queue: bool = False, filt: Optional[tuple] = None,
                    nd: int = 0) -> "_lib.T2SDecoder":
        """filt: (mode, k, thres) of filter_setting (default: the reference's top_k); nd: dialogue records behind the queue"""
        d, b = self.d, self.buf
        dec = _lib.T2SDecoder()
        dec.filter_mode, k, dec.top_p = filt or self._default_filter
        dec.n_dialogues = int(nd)
        dec.batch, dec.ctx_rows = batch, self.max_source + 2
        dec.cfg_scale = float(cfg_scale)
        dec.dim, dec.inner, dec.heads = d["dim_target"], d["inner"], d["heads"]
        dec.ff_inner, dec.ff_inner_pad, dec.depth = d["ff_tgt"], self.Fp, d["target_depth"]
        dec.streams, dec.vocab, dec.dim_emb = d["streams"], d["vocab"], d["dim_emb"]
        dec.n_ctx, dec.max_len, dec.top_k, dec.temperature = 0, self.max_length, k, float(temperature)
        dec.layers = C.cast(self._layers, C.POINTER(_lib.T2SLayer))
        dec.final_gamma, dec.emb = self.dec_final.data_ptr(), self.emb.data_ptr()
        dec.rope_cos, dec.rope_sin = self.rope[0].data_ptr(), self.rope[1].data_ptr()
        for n in ("uniforms", "x", "q", "att", "h", "logits", "tokens", "state"):
            setattr(dec, n, b[n].data_ptr())
        dec.uniform_steps = self._steps
        if queue:
            dec.queue, dec.dialogues, dec.start = b["queue"].data_ptr(), b["dialogues"].data_ptr(), self.start.data_ptr()
        return dec

    def _run_steps(self, temperature: float, batch: int, n: int, cfg_scale: float = 1.0, queue: bool = False, filt=None, nd: int = 0,
                   scored: bool = False, per: bool = False, mixed: Optional[int] = None, rules: bool = False) -> None:
        """n token steps on the current stream without a graph.  scored: cvx_t2s_decode_steps_scored (log-probs of every step's token into
        buf["logprobs"], forced dialogues honoured); else cvx_t2s_decode_steps, exactly as before that entry existed.
        per: cvx_t2s_decode_steps_per_dialogue - the settings come from buf["per"], one row per dialogue record; temperature and filt
        are not looked at and cfg_scale only says whether the slots run in guided pairs.
        mixed (with per and queue): cvx_t2s_decode_steps_mixed with that many guided utterances among the nd records - the pair layout
        comes from the records; n = 0 runs its scheduler alone, which arms idle slots.
        rules (with per): cvx_t2s_decode_steps_rules - that chain, or the mixed one, under the history rules of buf["rules"], one row per
        dialogue record."""
        lib, dec = _lib.load(), self._descriptor(temperature, batch, cfg_scale, queue, filt, nd)
        sc = C.byref(_lib.T2SScoring(C.sizeof(_lib.T2SScoring), self.max_length, self.buf["logprobs"].data_ptr())) if scored else None
        if not per:
            if scored:
                _lib.check(lib.cvx_t2s_decode_steps_scored(C.byref(dec), sc, n, ops._stream()), "cvx_t2s_decode_steps_scored")
            else:
                _lib.check(lib.cvx_t2s_decode_steps(C.byref(dec), n, ops._stream()), "cvx_t2s_decode_steps")
            return
        pd = _lib.T2SPerDialogue(C.sizeof(_lib.T2SPerDialogue), self.buf["per"].shape[0], self.buf["per"].data_ptr())
        if rules:
            mx = None if mixed is None else C.byref(_lib.T2SMixed(C.sizeof(_lib.T2SMixed), int(mixed)))
            ru = _lib.T2SRules(C.sizeof(_lib.T2SRules), self.buf["rules"].shape[0], self.buf["rules"].data_ptr())
            _lib.check(lib.cvx_t2s_decode_steps_rules(C.byref(dec), sc, C.byref(pd), mx, C.byref(ru), n, ops._stream()), "cvx_t2s_decode_steps_rules")
            return
        if mixed is not None:
            mx = _lib.T2SMixed(C.sizeof(_lib.T2SMixed), int(mixed))
            _lib.check(lib.cvx_t2s_decode_steps_mixed(C.byref(dec), sc, C.byref(pd), C.byref(mx), n, ops._stream()), "cvx_t2s_decode_steps_mixed")
            return
        _lib.check(lib.cvx_t2s_decode_steps_per_dialogue(C.byref(dec), sc, C.byref(pd), n, ops._stream()), "cvx_t2s_decode_steps_per_dialogue")

    def _uniform_view(self, n: int) -> torch.Tensor:
        """[n, steps, streams, vocab] view of the uniform draws of the first n dialogues"""
        S, V = self.d["streams"], self.d["vocab"]
        return self.buf["uniforms"][: n * self._steps * S * V].view(n, self._steps, S, V)

    def _slot_records(self, ctx, limit: int = 0, flags: int = 0) -> torch.Tensor:
        """slot records [slots, SR] (CPU): slot b decodes dialogue b from position 0; slots past len(ctx) idle at max_length"""
        rows = [[0, 0, 0, ctx[i], i, limit, flags, 0] if i < len(ctx) else [self.max_length, 1, 0, 1, 0, 0, 0, 0] for i in range(self._slots)]
        return torch.tensor(rows, dtype=torch.int32)


    def _read_state(self, nb: int) -> list:
        """slot records of the first nb slots (synchronises the current stream)."""
        return self.buf["state"].tolist()[:nb]

    # ---- the host looks at device-side records ONE CHUNK BEHIND the device
    def _mirror_setup(self) -> None:
        if self._stage is None:
            rows = max(self._slots, self._dialogues)
            self._stage = [torch.empty(rows, SR, dtype=torch.int32, device=self.device) for _ in range(2)]
            self._pin = [torch.empty(rows, SR, dtype=torch.int32).pin_memory() for _ in range(2)]
            self._stage_ev = [torch.cuda.Event(), torch.cuda.Event()]
            self._pin_ev = [torch.cuda.Event(), torch.cuda.Event()]
            self._helper = torch.cuda.Stream(device=self.device)

    def _mirror_push(self, k: int, src: torch.Tensor, via_helper: bool) -> None:
        """enqueue a copy of the records `src` [rows, SR] into pinned buffer k behind everything the current stream holds.
        On an ordinary stream: a non_blocking copy into pinned memory on the decode stream itself.  On a CU-masked stream of
        ops.CUPartition that form is NOT used: torch's pinned-memory allocator remembers the stream of such a copy, and a masked stream
        destroyed at exit before the block is freed takes the process down (tools/archive/cu_mask_exit_probe.py) - there the record is copied
        device-to-device on the decode stream and a plain helper stream brings it to the host."""
        rows = src.shape[0]
        if via_helper:
            self._stage[k][:rows].copy_(src)
            self._stage_ev[k].record()
            with torch.cuda.stream(self._helper):
                self._helper.wait_event(self._stage_ev[k])
                self._pin[k][:rows].copy_(self._stage[k][:rows], non_blocking=True)
                self._pin_ev[k].record()
        else:
            self._pin[k][:rows].copy_(src, non_blocking=True)
            self._pin_ev[k].record()

    def _mirror_pull(self, k: int, rows: int) -> list:
        self._pin_ev[k].synchronize()
        return self._pin[k][:rows].tolist()

    def _chunks(self, replay, records, rows: int, done, cap: int):
        """Chunks of CHUNK token steps - one `replay()` each - until `done(rows_list)` says so, at most `cap` of them.
        The host looks at the device-side records ONE CHUNK BEHIND the device: records[:rows] of chunk i are copied between the replays of
        chunks i and i + 1 and read (`done`) while chunk i + 1 runs - the decode chain never waits for a host round trip (nor for a host
        thread that is waiting for the interpreter lock while another thread drives the acoustic solve, pipeline.py); the price is
        at most one chunk decoded past the last end (masked afterwards like every token behind an eos).  A loop that ends at the cap
        hands the last chunk's records to `done` as well.  -> (chunks run, the last rows read)."""
        self._mirror_setup()
        via_helper = ops.is_partition_stream()
        i, pulled, ended = 0, None, False
        while i < cap and not ended:
            replay()
            self._mirror_push(i & 1, records[:rows], via_helper)
            if i:
                pulled = self._mirror_pull((i - 1) & 1, rows)
                ended = done(pulled)
            i += 1
        if i and not ended:
            pulled = self._mirror_pull((i - 1) & 1, rows)
            done(pulled)
        if i:
            self._pin_ev[(i - 1) & 1].synchronize()  # (the last PUSHED buffer, read or not: the helper stream's last copy - the next call reuses the buffers)
        return i, pulled

    def _capture(self, key: tuple, launch, idle):
        """The graph stored under `key`, captured on first use: `launch()` (CHUNK steps) runs once outside the capture (module load, kernel
        attributes) and once inside it, both on the state `idle()` sets up, on which the steps do nothing."""
        g = self._graphs.get(key)
        if g is not None:
            return g
        idle()
        launch()                                       # warm-up outside capture
        cur = torch.cuda.current_stream()
        if self._cap is None:
            self._cap = torch.cuda.Stream(device=self.device)
        ops.saturation_share(cur, self._cap)           # (the capture stream belongs to this call: flag and CU count of `cur`)
        with ops.CAPTURE_GATE.exclusive():             # (no other entry point of the package syncs / copies meanwhile)
            cur.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self._cap, capture_error_mode="thread_local"):
                launch()
        if len(self._graphs) >= 8:
            self._graphs.clear()
        self._graphs[key] = g
        return g

    def _graph(self, temperature: float, batch: int, cfg_scale: float = 1.0, queue: bool = False, filt=None, nd: int = 0, scored: bool = False,
               per: bool = False, mixed: Optional[int] = None, rules: bool = False):
        """The captured graph of CHUNK token steps for this (batch, stream CU count, mode, filter, scoring); captured on first use.  (nd, the
        number of dialogue records, is only validated by the C call: it is not part of the key.)  Capturing runs the
        steps once outside the capture (module load, kernel attributes): callers get their graph BEFORE they set up the decode state -
        the warm-up runs on idle slot records (position max_length: the sampling kernel returns at once, every other kernel clamps).
        per: the per-dialogue chain, whose settings live in a device table - its key carries a "per" marker INSTEAD of (temperature, scale,
        filter), so one graph per (batch, CUs, guided?, queue, scored) serves every mix of settings.
        mixed: the mixed chain (cvx_t2s_decode_steps_mixed) - its key is ("mixed", batch, CUs, scored): the launches depend on neither the
        settings nor on how many utterances are guided.
        rules: the per-dialogue or mixed chain under the history rules (cvx_t2s_decode_steps_rules) - the key gains a "rules" marker, not
        the values: they live in a device table too, and one graph serves every mix of rules."""
        filt = filt or self._default_filter
        key = (temperature, batch, cfg_scale, ops.stream_cus(), queue, self._gen, filt, bool(scored))   # (the kernels' shape follows the CUs the stream owns)
        if per:
            key = ("per", batch, cfg_scale > 1.0, ops.stream_cus(), queue, self._gen, bool(scored))
        if mixed is not None:
            key = ("mixed", batch, ops.stream_cus(), self._gen, bool(scored))
        if rules:
            key += ("rules",)

        def idle():
            self.buf["state"].copy_(self._slot_records([]))
            if mixed is not None:                      # (the scheduler of the warm-up steps must find nothing to hand out)
                self.buf["queue"].zero_()
        return self._capture(key, lambda: self._run_steps(temperature, batch, CHUNK, cfg_scale, queue, filt, nd, scored, per, mixed, rules), idle)

    def _run_chunk(self, temperature: float, batch: int = 1, cfg_scale: float = 1.0, queue: bool = False, filt=None, nd: int = 0,
                   scored: bool = False, per: bool = False, mixed: Optional[int] = None, rules: bool = False) -> None:
        """CHUNK token steps on the current stream: a graph replay of the per-launch path (the graph must exist - `_graph` - unless
        CVX_GRAPH=0 asks for plain launches)."""
        if os.environ.get("CVX_GRAPH", "1") != "1":
            self._run_steps(temperature, batch, CHUNK, cfg_scale, queue, filt, nd, scored, per, mixed, rules)
            return
        self._graph(temperature, batch, cfg_scale, queue, filt, nd, scored, per, mixed, rules).replay()

    def _contexts(self, sources, rows=None) -> list:
        """encoder + the cross-attention k/v of the utterances into dialogue rows `rows` (default 0, 1, ...): [null | to_kv(enc)]
        -> context rows per utterance.  One packed encoder pass and one to_kv GEMM per decoder layer for all of them."""
        n = len(sources)
        rows = list(range(n)) if rows is None else list(rows)
        enc, rg = self.encode_many(sources)
        R = self.max_source + 2
        dst = torch.cat([torch.arange(t, dtype=torch.int64) + (rows[i] * R + 1) for i, t in enumerate(rg.lengths)])
        dst = ops.h2d(dst, self.device)
        first = ops.h2d(torch.tensor([r * R for r in rows], dtype=torch.int64), self.device)
        kv = torch.empty(rg.M, 2 * self.d["inner"], dtype=torch.float32, device=self.device)
        for L in self.dec:
            ops.gemm(enc, L["wkv_c"], kv)
            flat = L["kv_c"].view(-1, kv.shape[1])
            flat.index_copy_(0, dst, kv)
            flat.index_copy_(0, first, L["null"][None, :].expand(n, -1))
        return [t + 1 for t in rg.lengths]

    def _guided_contexts(self, sources) -> list:
        """`_contexts` for guided utterances, a pair of dialogue rows each: the context of utterance u into row 2u, and into row 2u + 1 the
        null key / value row only = every context key masked out.  -> context rows per dialogue row, [c0, 1, c1, 1, ...]"""
        n, ctx = len(sources), []
        for c in self._contexts(sources, range(0, 2 * n, 2)):
            ctx += [c, 1]
        for L in self.dec:
            L["kv_c"][1:2 * n:2, 0].copy_(L["null"][None, :].expand(n, -1))
        return ctx

    def _mask_after_eos(self, streams: torch.Tensor):
        """(flat tokens, streams) of the token rows [S, length] of one utterance: a copy of the rows, and their tokens stream after stream
        without what lies behind a stream's first eos - mask_after_eos (text2semantic.py:73-76)"""
        streams = streams.clone()
        after = (streams == self.d["vocab"] - 1).cumsum(dim=-1) > 0
        after = torch.nn.functional.pad(after, (1, -1), value=False)
        flat = streams.masked_fill(after, PAD_ID).reshape(-1)
        return flat[flat != PAD_ID], streams

    def _cut(self, j: int, length: int, logits=None, logprobs: bool = False):
        """(flat tokens, streams[, logits][, logprobs]) of dialogue row j after `length` steps"""
        item = self._mask_after_eos(self.buf["tokens"][j, :, :length])
        if logits is not None:
            item += (logits[:length],)
        if logprobs:
            item += (self.buf["logprobs"][j, :, :length].clone(),)
        return item

    @ops.gated
    @torch.no_grad()          # (not inference_mode: tensors torch creates lazily during the first graph capture,
                              #  e.g. the generator's graph-safe state, would become inference tensors)
    def generate_batch(self, sources, uniforms=None, max_length: Optional[int] = None, temperature: float = 1.0,
                       generator: Optional[torch.Generator] = None, collect_logits: bool = False, cond_scale: float = 1.0,
                       ignore_eos: bool = False, filter_logits_fn="top_k", filter_fn_kwargs=None, return_logprobs: bool = False,
                       repetition_penalty: float = 1.0, repetition_window: int = 0, no_repeat_ngram_size: int = 0, min_length: int = 0):
        """Decode up to MAX_BATCH utterances together IN LOCK STEP (all start at position 0; the batch runs until the last one has
        sampled its eos).  sources: list of [n] / [1, n] id tensors; uniforms: optional list of [steps, streams, vocab] tensors (one
        per utterance).  Returns a list of (flat tokens, streams[, logits]) tuples, each exactly what `generate` returns for that
        utterance alone.  (`generate_many`: any number of utterances through continuously refilled slots.)
        ignore_eos (benchmarks: a fixed amount of work): decode max_length steps whatever is sampled; `streams` then holds all of them.
        cond_scale > 1: classifier-free guidance (text2semantic.py:780-792; one-output models, up to MAX_BATCH / 2 utterances):
        every utterance takes two decode slots - the text context and the context masked out (cross-attention then sees the
        learned null key / value only) - and each step samples from null + (cond - null) * cond_scale; logits returned under
        collect_logits are the COMBINED ones, null + (cond - null) * cond_scale (what the reference filters and samples from).
        filter_logits_fn / filter_fn_kwargs: the logit filter, as TextToSemantic.generate takes it (`filter_setting`); the default is
        the reference's top_k with k = ceil(0.1 * vocab).
        return_logprobs: every result gains, as its LAST entry, a float32 [S, length] tensor aligned with `streams`: the log-probability
        the model gave each sampled token - log_softmax of the row the filter sees (the guidance-combined logits under cond_scale > 1),
        before the filter, the temperature and the noise (include/covomix_hip.h).  Off (the default) nothing changes.
        repetition_penalty / repetition_window / no_repeat_ngram_size / min_length: the HISTORY RULES (`check_rules`; the definition:
        include/covomix_hip.h, cvx_t2s_decode_steps_rules) - per output stream, from the tokens the stream has emitted so far: every id
        seen in its last `repetition_window` tokens (0: all) is penalised once (l > 0 ? l / penalty : l * penalty), an id that would
        complete an n-gram the stream already holds is not selectable, and neither is the eos below min_length.  They act on the row
        the filter sees, before the filter; logits under collect_logits and log-probs under return_logprobs stay those of the row
        BEFORE the rules (so the log-probs still equal score_many of the tokens).  All off (the defaults): the call as it was, graph for
        graph; any on: the per-dialogue chain under a rules table with equal rows (cvx_t2s_decode_steps_rules)."""
        S, V = self.d["streams"], self.d["vocab"]
        filt = filter_setting(filter_logits_fn, filter_fn_kwargs, V)
        rules = check_rules(None, len(sources), self._rule_bound(max_length), repetition_penalty, repetition_window, no_repeat_ngram_size,
                            min_length)
        ruled = rules_active(rules)
        guided = float(cond_scale) > 1.0
        if guided and S != 1:
            raise NotImplementedError("guidance (cond_scale > 1) on a two-output model: the reference feeds the full-width hidden "
                                      "state to the half-width logit head there (text2semantic.py:783-785) and cannot run")
        P = 2 if guided else 1    # decode slots (and dialogue rows) per utterance: utterance u decodes in slot P u, its null context in P u + 1
        scale = float(cond_scale) if guided else 1.0
        n = len(sources)
        if not 1 <= n <= MAX_BATCH // P:
            raise ValueError(f"1..{MAX_BATCH // P} utterances per {'guided ' if guided else ''}decode batch, got {n}")
        nb = P * n
        max_len = min(int(max_length or self.max_length), self.max_length)
        us = None
        if uniforms is not None:
            us = [u.to(self.device, torch.float32).reshape(u.shape[0], S, V) for u in uniforms]
            max_len = min([max_len] + [u.shape[0] for u in us])
        scored, temperature = bool(return_logprobs), float(temperature)
        self._ensure(nb, nb, max_len, scored)
        b = self.buf
        if not collect_logits and max_len > 0:
            self._graph(temperature, nb, scale, False, filt, 0, scored, ruled, None, ruled)
        if ruled:                 # the settings and the rules as table rows, one per slot (slot b decodes dialogue b; a null half mirrors its text half)
            resolved = check_settings([None] * n, n, V, S, temperature, filter_logits_fn, filter_fn_kwargs, scale)
            b["per"][:nb].copy_(ops.h2d(settings_rows(resolved).repeat_interleave(P, dim=0), self.device))
            b["rules"][:nb].copy_(ops.h2d(rules_rows(rules).repeat_interleave(P, dim=0), self.device))
        ctx = self._guided_contexts(sources) if guided else self._contexts(sources)
        uview = self._uniform_view(nb)[0::P]
        if us is None:            # (drawn step-major, as the [steps, batch, streams, vocab] buffer of earlier versions was: same seeds, same tokens)
            uview[:, :max_len].copy_(torch.rand(max_len, n, S, V, device=self.device, generator=generator).permute(1, 0, 2, 3))
        else:
            for i, u in enumerate(us):
                uview[i, :max_len].copy_(u[:max_len])
        b["x"][:nb].copy_(self.start[None, :].expand(nb, -1))
        b["state"].copy_(self._slot_records(ctx))
        logits = []
        st = self._slot_records(ctx).tolist()[:nb]
        done = lambda st: all(st[r][1] for r in range(0, nb, P)) and not ignore_eos
        if collect_logits:                                              # (tests: one step at a time without a graph)
            for _ in range(max_len):
                self._run_steps(temperature, nb, 1, scale, False, filt, 0, scored, ruled, None, ruled)
                lg = b["logits"][:nb].clone()
                logits.append(lg[1::2] + (lg[0::2] - lg[1::2]) * scale if guided else lg)
                st = self._read_state(nb)
                if done(st):
                    break
        elif max_len > 0:
            self._chunks(lambda: self._run_chunk(temperature, nb, scale, False, filt, 0, scored, ruled, None, ruled), b["state"], nb, done,
                         (max_len + CHUNK - 1) // CHUNK)
            st = self._read_state(nb)
        out = []
        for u in range(n):
            r = st[P * u]
            length = min(r[2] if r[1] and r[2] <= max_len and not ignore_eos else max_len, max_len)
            out.append(self._cut(P * u, length, torch.stack([lg[u] for lg in logits]) if collect_logits and logits else None, scored))
        return out

    def _forced_tokens(self, forced, n: int, scored: bool):
        """`forced` of generate_many: None when no utterance is forced, else the list with every entry given as an int64 [S, L] host tensor
        (`check_targets`)"""
        if forced is not None:
            if not scored or len(forced) != n:
                raise ValueError("forced: one entry per utterance, with return_logprobs=True")
            if all(f is None for f in forced):
                forced = None
        if forced is not None:
            forced = list(forced)
            fi = [j for j in range(n) if forced[j] is not None]
            for j, t in zip(fi, check_targets([forced[j] for j in fi], self.d["streams"], self.d["vocab"], self.max_length)):
                forced[j] = t
        return forced

    def _step_limits(self, n: int, uniforms, max_length, limits, forced):
        """-> (us, max_len, lim, span, is_forced) of a generate_many window: the caller's draws on the device (None: none given; an entry is
        None for a forced utterance without draws), the steps of the call (the shortest draws bound it), the step limit of every utterance
        (a forced one: the length of its tokens) and the steps an utterance can take: the rows of the pinned result buffers"""
        S, V = self.d["streams"], self.d["vocab"]
        max_len = min(int(max_length or self.max_length), self.max_length)
        us = None
        is_forced = [forced is not None and forced[j] is not None for j in range(n)]
        if uniforms is not None:
            us = [None if (u is None and is_forced[j]) else u.to(self.device, torch.float32).reshape(u.shape[0], S, V) for j, u in enumerate(uniforms)]
            max_len = min([max_len] + [u.shape[0] for u in us if u is not None])
        lim = [max_len] * n if limits is None else [max(1, min(int(x), max_len)) for x in limits]
        if max_len <= 0:
            raise ValueError("generate_many needs at least one step")
        span = max_len
        if forced is not None:
            lim = [forced[j].shape[1] if is_forced[j] else lim[j] for j in range(n)]
            span = max(span, max(lim))
        return us, max_len, lim, span, is_forced

    def _queue_chunks(self, replay, nrec: int, text: list, lim: list, span: int, scored: bool, on_done, last_records) -> list:
        """The chunks (`_chunks`) of a generate_many window whose state is set up, until the dialogue records show every utterance finished
        (status >= 2) -> the results.  Utterance j is carried by record text[j]; last_records(records) is what `last_records` keeps of
        the records read (tests / tools: status, steps and slot of every utterance).
        Token rows of finished utterances reach the host through the helper stream into pinned memory (a dialogue's rows are final
        once the host has SEEN it finished: any stream may read them) and are cut on the host - nothing here makes the decode
        stream wait, so the chunks stay back to back (a device-side boolean index per utterance cost a stream sync each: 64
        utterances on 64 slots ran 996 ms against 746 ms in lock step)"""
        n, S, b = len(text), self.d["streams"], self.buf
        self._mirror_setup()                               # (the helper stream)
        out: list = [None] * n
        seen = [False] * n
        tok_pin = torch.empty(n, S, span, dtype=torch.int64).pin_memory()
        lp_pin = torch.empty(n, S, span, dtype=torch.float32).pin_memory() if scored else None
        copies: list = []                                  # (j, steps, event) in flight on the helper stream

        def finish(block: bool):
            while copies and (block or copies[0][2].query()):
                j, length, ev = copies.pop(0)
                ev.synchronize()
                out[j] = self._mask_after_eos(tok_pin[j, :, :length])
                if scored:
                    out[j] += (lp_pin[j, :, :length].clone(),)
                if on_done is not None:
                    on_done(j, out[j])

        def collect(records) -> bool:
            self.last_records = last_records(records)
            fresh = [j for j in range(n) if not seen[j] and records[text[j]][3] >= 2]
            if fresh:
                with torch.cuda.stream(self._helper):
                    for j in fresh:
                        seen[j] = True
                        length = records[text[j]][4]
                        tok_pin[j, :, :length].copy_(b["tokens"][text[j], :, :length], non_blocking=True)
                        if scored:
                            lp_pin[j, :, :length].copy_(b["logprobs"][text[j], :, :length], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record()
                        copies.append((j, length, ev))
            finish(False)
            return all(seen)
        cap = (sum(lim) + CHUNK - 1) // CHUNK + 4          # (one slot decoding everything: cannot be reached)
        i, _ = self._chunks(replay, b["dialogues"], nrec, collect, cap)
        finish(True)
        if not all(seen):
            raise RuntimeError(f"text2semantic continuous decode: {seen.count(False)} of {n} utterances did not finish in {i} chunks")
        return out

    @ops.gated
    @torch.no_grad()
    def generate_many(self, sources, uniforms=None, max_length: Optional[int] = None, temperature: float = 1.0,
                      generator: Optional[torch.Generator] = None, slots: int = 32, ignore_eos: bool = False, limits=None, on_done=None,
                      cond_scale: float = 1.0, filter_logits_fn="top_k", filter_fn_kwargs=None, return_logprobs: bool = False, forced=None,
                      settings=None, prefixes=None, mixed_guidance: bool = False, repetition_penalty: float = 1.0, repetition_window: int = 0,
                      no_repeat_ngram_size: int = 0, min_length: int = 0, prefill: bool = False):
        """Decode ANY number of utterances through `slots` decode slots with continuous batching: every utterance runs the
        reference's loop (text2semantic.py:749-848) from position 0 to its first eos (:803-818) or its step limit, and the slot it
        ran in takes the next pending utterance in the sampling kernel of that very step (cvx_t2s_decoder.queue) - utterances end
        at different steps, and a lock-step batch would run half empty.  Every utterance gets exactly the tokens it gets alone.
        sources / uniforms as generate_batch; limits: optional per-utterance step limits (default max_length for all).
        on_done(j, (flat, streams)): called for utterance j as soon as the host has seen it finish (the host reads the dialogue
        records one chunk of CHUNK steps behind the device) - the next pipeline stage can start on the first results while the
        rest decodes.  Returns the list of (flat tokens, streams) in input order - int64 tensors ON THE HOST (they travel through pinned
        memory on a helper stream so that nothing makes the decode stream wait).
        cond_scale > 1 (classifier-free guidance, one-output models): an utterance takes a PAIR of decode slots (text context / null
        context) and a pair of dialogue records; the even slot of a pair ends the utterance and refills both (include/covomix_hip.h).
        At most MAX_BATCH / 2 utterances are in flight (`slots` still counts slots: slots // 2 pairs), and WINDOW counts dialogue
        records, so a window holds WINDOW / 2 guided utterances.  limits, ignore_eos, on_done and last_records keep their meaning
        per utterance (last_records: the record of the text-context half; its slot is the even slot of the pair).
        filter_logits_fn / filter_fn_kwargs: as generate_batch.
        return_logprobs: every result gains a float32 [S, length] host tensor aligned with `streams` (generate_batch), through the same
        pinned-memory path as the tokens.  Off, nothing changes.
        forced (with return_logprobs; `score_many` is the public form): a list with, per utterance, None (sampled as usual) or int64
        [S, L] tokens to SCORE instead of sampling - a forced dialogue (include/covomix_hip.h): the steps read these tokens, draw no
        uniforms (that utterance's entry of `uniforms` may be None), ignore every eos and stop after L steps whatever `limits` says;
        its `streams` are the tokens given.  Forced and sampled utterances share the queue and the slots.
        settings (default None: the call as it always was, graph for graph): one entry per utterance - None, a mapping or an
        UtteranceSettings with any of temperature, filter_logits_fn, filter_fn_kwargs, cond_scale; what an entry leaves out takes the
        call's scalar (`check_settings`).  Utterances with different settings share the slots, the queue and ONE captured graph: the
        sampling kernel reads the settings of the dialogue a slot decodes from a device table (cvx_t2s_decode_steps_per_dialogue), and
        every utterance gets, bit for bit, what it gets alone with its settings as the call's scalars.  Guided and unguided utterances do
        not share a call (ValueError): the slot-pair layout belongs to the launch - unless mixed_guidance (below) is on.
        prefixes (default None): one entry per utterance - None, or int64 [S, P] tokens, 1 <= P < that utterance's step limit, none of
        them an eos (`check_prefixes`): the decode CONTINUES from them.  They are copied into the utterance's token row; its first P steps
        read them instead of sampling (no uniforms are read there; the uniforms stay indexed by position), and from position P on it
        samples as ever - so a prefix cut from an earlier result, with the same uniforms, reproduces the rest of that result.  `streams`
        starts with the prefix; under return_logprobs the positions below P hold the prefix tokens' teacher-forced log-probs (what
        score_many gives them).  A prefix for a forced utterance is a ValueError.
        mixed_guidance (default False: nothing changes, graph for graph): guided and unguided utterances share the call, the slots, the
        queue and one captured graph (cvx_t2s_decode_steps_mixed).  cond_scale is then only the default of `settings`: an utterance whose
        scale is exactly 1 is unguided and takes one dialogue record and one slot, one whose scale is > 1 is guided and takes two records
        and two slots - ANY two: a one-block scheduler launch behind every sampling launch hands the idle slots out in queue order, and a
        guided utterance at the head waits until two are idle (`mixed_schedule` replays that policy).  `slots` counts slots and must be
        >= 2 when any utterance is guided; WINDOW counts records, and windows are cut on utterance boundaries (`mixed_windows`).
        last_records stays one record per utterance (that of the text half) and gains, as a ninth entry, the slot of the null half of a
        guided utterance (None for an unguided one).  Every other argument keeps its meaning, and every utterance gets, bit for bit, what
        it gets alone.
        repetition_penalty / repetition_window / no_repeat_ngram_size / min_length (generate_batch): the history rules, as scalars for
        the call; the entries of `settings` may name them per utterance (`check_rules`).  With every rule off the call is what it was,
        graph for graph.  With any on, the call runs the per-dialogue (or mixed) chain under a rules table
        (cvx_t2s_decode_steps_rules) and ONE graph serves every mix; an utterance's history is its own token row, so a refilled slot
        inherits nothing and every utterance still gets, bit for bit, what it gets alone with its rules.  A prefix counts as history;
        given steps (prefix, forced) are not subject to the rules.
        prefill (default False; with no prefix in the call it changes nothing, graph for graph): the first P positions of every prefixed
        utterance come from ONE causal full-sequence pass (`_prefill`; include/covomix_hip.h, cvx_t2s_prefill_attention_f32) instead of P
        decode steps: the pass fills the caches of the utterance's slot(s) - both of a guided pair - for positions 0 .. P - 1, its slot
        record starts at position P with the embedding of the prefix' last tokens as input, its token row holds the prefix (history rules
        and `streams` as ever), and under return_logprobs the positions below P hold the pass' log-probs.  The device-side refill always
        starts a dialogue at position 0 with an empty cache, so such a call is cut into windows of at most (armed slots / slots per
        utterance) utterances, each an ordinary queue call in which the host arms every slot - nothing is refilled: MANY SHORT prefixes
        may be better off without prefill.  The prefix positions are fp32-class, not bit-identical to the step chain (score_many).
        ValueError with mixed_guidance, and for a model whose widths the full-sequence kernels do not admit (`_prefill_check`)."""
        if prefill and mixed_guidance:
            raise ValueError("generate_many: prefill=True does not run with mixed_guidance=True (the mixed pool's slots are armed on the device)")
        rule_kw = dict(repetition_penalty=repetition_penalty, repetition_window=repetition_window, no_repeat_ngram_size=no_repeat_ngram_size,
                       min_length=min_length)
        if mixed_guidance:
            return self._generate_many_mixed(sources, uniforms, max_length, temperature, generator, slots, ignore_eos, limits, on_done,
                                             cond_scale, filter_logits_fn, filter_fn_kwargs, return_logprobs, forced, settings, prefixes, rule_kw)
        d = self.d
        S, V = d["streams"], d["vocab"]
        n = len(sources)
        scored = bool(return_logprobs)
        forced = self._forced_tokens(forced, n, scored)
        filt = filter_setting(filter_logits_fn, filter_fn_kwargs, V)
        cond_scale = float(cond_scale)
        cfg = cond_scale > 1.0
        if cfg and S != 1:
            raise NotImplementedError("guidance (cond_scale > 1) on a two-output model: the reference cannot run it (generate_batch)")
        P = 2 if cfg else 1       # dialogue records (and decode slots) per utterance
        rules = check_rules(settings, n, self._rule_bound(max_length), **rule_kw)
        ruled = rules_active(rules)
        per = settings is not None or prefixes is not None or ruled
        resolved = None
        if per:                   # (validated for the whole call before any window runs)
            resolved = check_settings([None] * n if settings is None else settings, n, V, S, temperature, filter_logits_fn, filter_fn_kwargs,
                                      cond_scale)
            if prefixes is not None and len(list(prefixes)) != n:
                raise ValueError(f"prefixes: {len(list(prefixes))} entries for {n} utterances")
        if n == 0:
            return []
        win = WINDOW // P
        use_prefill = bool(prefill) and prefixes is not None and any(p_ is not None for p_ in prefixes)
        if use_prefill:           # (the host arms every slot of such a window: as many utterances as slots hold)
            self._prefill_check()
            win = max(1, min(int(slots) // P, MAX_BATCH // P))
        if n > win:               # (the context k/v, uniforms and token rows of every queued utterance are resident: bounded windows)
            out = []
            for w in range(0, n, win):
                out += self.generate_many(sources[w:w + win], None if uniforms is None else uniforms[w:w + win], max_length, temperature,
                                          generator, slots, ignore_eos, None if limits is None else limits[w:w + win],
                                          None if on_done is None else (lambda j, r, w=w: on_done(w + j, r)),
                                          cond_scale, filter_logits_fn, filter_fn_kwargs, return_logprobs,
                                          None if forced is None else forced[w:w + win],
                                          None if settings is None else list(settings)[w:w + win],
                                          None if prefixes is None else list(prefixes)[w:w + win], **rule_kw, prefill=prefill)
            return out
        nb = P * max(1, min(int(slots) // P, MAX_BATCH // P, n))
        nb = nb if nb in (1, 2, 4) else min((nb + 7) // 8 * 8, MAX_BATCH)      # whole kernel groups (idle slots cost nothing)
        nrec = P * n
        text = list(range(0, nrec, P))                     # the record that carries utterance j
        us, max_len, lim, span, is_forced = self._step_limits(n, uniforms, max_length, limits, forced)
        pre = check_prefixes([None] * n if prefixes is None else prefixes, n, S, V, lim, forced) if per else [None] * n
        self._ensure(nb, nrec, max_len, scored)
        b = self.buf
        temperature = float(temperature)
        self._graph(temperature, nb, cond_scale, True, filt, nrec, scored, per, None, ruled)
        ctx = self._guided_contexts(sources) if cfg else self._contexts(sources)
        uview = self._uniform_view(nrec)[0::P]            # the draws of utterance j live in its first record
        if us is None:
            if not all(is_forced):                         # (a forced dialogue reads no draws: a pure scoring call draws none)
                uview[:, :max_len].copy_(torch.rand(n, max_len, S, V, device=self.device, generator=generator))
        else:
            for j, u in enumerate(us):
                if u is not None:
                    uview[j, :max_len].copy_(u[:max_len])
        flags = [_lib.T2S_FLAG_FORCED if is_forced[j] else (_lib.T2S_FLAG_IGNORE_EOS if ignore_eos else 0) for j in range(n)]
        if forced is not None:                             # the token row of a forced dialogue holds its tokens before its first step
            for j in range(n):
                if is_forced[j]:
                    b["tokens"][text[j], :, :lim[j]].copy_(ops.h2d(forced[j], self.device))
        if per:                                            # one settings row per dialogue record (the odd record of a pair mirrors the even one)
            b["per"][:nrec].copy_(ops.h2d(settings_rows(resolved, [0 if p is None else p.shape[1] for p in pre]).repeat_interleave(P, dim=0),
                                          self.device))
            for j, p in enumerate(pre):                    # the token row of a prefixed dialogue holds the prefix before its first step
                if p is not None:
                    b["tokens"][text[j], :, :p.shape[1]].copy_(ops.h2d(p, self.device))
        if ruled:
            b["rules"][:nrec].copy_(ops.h2d(rules_rows(rules).repeat_interleave(P, dim=0), self.device))
        first = min(nb, nrec)     # records (= slots) that start at once; whole pairs under guidance (nb and nrec are even)
        rec = torch.tensor([[ctx[r], lim[r // P], flags[r // P], 1 if r < first else 0, 0, r if r < first else 0, 0, 0] for r in range(nrec)],
                           dtype=torch.int32)
        b["dialogues"][:nrec].copy_(rec)
        b["queue"].copy_(torch.tensor([first, nrec], dtype=torch.int32))
        slot = self._slot_records(ctx[:first]).clone()
        for r in range(first):
            slot[r, 5], slot[r, 6] = lim[r // P], flags[r // P]
        b["x"][:first].copy_(self.start[None, :].expand(first, -1))
        if use_prefill:           # (first == nrec: every record sits in the slot of its own number)
            self._prefill_slots(pre, text, ctx, [r[2] for r in resolved], P, slot, scored)
        b["state"].copy_(slot)
        return self._queue_chunks(lambda: self._run_chunk(temperature, nb, cond_scale, True, filt, nrec, scored, per, None, ruled), nrec, text, lim,
                                  span, scored, on_done, lambda records: records[0::P])

    def _prefill_slots(self, pre, text, ctx, scales, P: int, slot: torch.Tensor, scored: bool) -> None:
        """generate_many(prefill=True), one window whose slots the host arms (record r in slot r): the prefixes `pre` (None: none) of the
        utterances in records text[j] (P = 2: the null half in text[j] + 1) run as prefill passes of at most PREFILL_ROWS rows that fill
        the slots' caches; the slot records `slot` (host) then start at the prefix length, the slots' x rows hold the embedding of the
        prefix' last tokens and, scored, the log-prob rows of the text records hold the passes' log-probs below it."""
        b, dev = self.buf, self.device
        idx = [j for j, p_ in enumerate(pre) if p_ is not None]
        for w0, w1 in prefill_windows([pre[j].shape[1] * P for j in idx]):
            js = idx[w0:w1]
            seqs, nulls = self._prefill_pairs([pre[j] for j in js], [text[j] for j in js], [ctx[text[j]] for j in js],
                                              [scales[j] if P == 2 else 1.0 for j in js], True)
            lps = self._prefill(seqs, nulls, [scales[j] for j in js], cache=True)
            for j, lp in zip(js, lps):
                if scored:
                    b["logprobs"][text[j], :, :lp.shape[1]].copy_(lp)
        last = ops.h2d(torch.stack([pre[j][:, -1] for j in idx]).reshape(-1), dev)        # [len(idx) * S] token ids
        xs = self.emb.index_select(0, last).view(len(idx), self.d["dim_target"])
        for h in range(P):
            rows = [text[j] + h for j in idx]
            b["x"].index_copy_(0, ops.h2d(torch.tensor(rows, dtype=torch.int64), dev), xs)
            for j in idx:
                slot[text[j] + h, 0] = pre[j].shape[1]

    def _generate_many_mixed(self, sources, uniforms, max_length, temperature, generator, slots, ignore_eos, limits, on_done, cond_scale,
                             filter_logits_fn, filter_fn_kwargs, return_logprobs, forced, settings, prefixes, rule_kw=None):
        """generate_many(mixed_guidance=True): the records are laid out by prefix sum (`mixed_records`: one per unguided utterance; text
        half and null half per guided one), everything that belongs to an utterance - uniforms, tokens, log-probs, prefix, forced tokens -
        lives in its text record, the settings row is mirrored onto the null record, and the slots are armed by the device's scheduler (a
        0-step call on idle slots), so the hand-out policy exists in one place."""
        d = self.d
        S, V = d["streams"], d["vocab"]
        n = len(sources)
        scored = bool(return_logprobs)
        forced = self._forced_tokens(forced, n, scored)
        filter_setting(filter_logits_fn, filter_fn_kwargs, V)
        resolved = check_settings([None] * n if settings is None else settings, n, V, S, temperature, filter_logits_fn, filter_fn_kwargs,
                                  float(cond_scale), mixed=True)
        rules = check_rules(settings, n, self._rule_bound(max_length), **(rule_kw or {}))
        ruled = rules_active(rules)
        if prefixes is not None and len(list(prefixes)) != n:
            raise ValueError(f"prefixes: {len(list(prefixes))} entries for {n} utterances")
        kinds = [r[2] > 1.0 for r in resolved]
        if any(kinds) and int(slots) < 2:
            raise ValueError(f"slots = {slots}: a guided utterance takes two decode slots")
        if n == 0:
            return []
        wins = mixed_windows(kinds)
        if len(wins) > 1:          # (the context k/v, uniforms and token rows of every queued record are resident: bounded windows)
            out, recs = [], []
            cut = lambda x, w0, w1: None if x is None else list(x)[w0:w1]
            for w0, w1 in wins:
                out += self._generate_many_mixed(sources[w0:w1], cut(uniforms, w0, w1), max_length, temperature, generator, slots, ignore_eos,
                                                 cut(limits, w0, w1), None if on_done is None else (lambda j, r, w0=w0: on_done(w0 + j, r)),
                                                 cond_scale, filter_logits_fn, filter_fn_kwargs, return_logprobs, cut(forced, w0, w1),
                                                 cut(settings, w0, w1), cut(prefixes, w0, w1), rule_kw)
                recs += self.last_records
            self.last_records = recs
            return out
        first = mixed_records(kinds)
        nrec, ng = first[-1], sum(kinds)
        text = first[:-1]                                      # the record that carries utterance j
        nulls = [text[j] + 1 for j in range(n) if kinds[j]]
        nb = max(1, min(int(slots), MAX_BATCH, nrec))
        us, max_len, lim, span, is_forced = self._step_limits(n, uniforms, max_length, limits, forced)
        pre = check_prefixes([None] * n if prefixes is None else prefixes, n, S, V, lim, forced)
        self._ensure(nb, nrec, max_len, scored)
        b = self.buf
        self._graph(1.0, nb, 1.0, True, None, nrec, scored, True, ng, ruled)
        ctx_text = self._contexts(sources, text)
        ctx = [1] * nrec
        for j in range(n):
            ctx[text[j]] = ctx_text[j]
        if nulls:                  # the null half: the learned null key / value row only (every context key masked out)
            ni = ops.h2d(torch.tensor(nulls, dtype=torch.int64), self.device)
            for L in self.dec:
                L["kv_c"][:, 0].index_copy_(0, ni, L["null"][None, :].expand(len(nulls), -1))
        uall = self._uniform_view(nrec)                        # the draws of utterance j live in its text record
        if us is None:
            if not all(is_forced):                             # (a forced dialogue reads no draws: a pure scoring call draws none)
                ti = ops.h2d(torch.tensor(text, dtype=torch.int64), self.device)
                uall[:, :max_len].index_copy_(0, ti, torch.rand(n, max_len, S, V, device=self.device, generator=generator))
        else:
            for j, u in enumerate(us):
                if u is not None:
                    uall[text[j], :max_len].copy_(u[:max_len])
        flags = [(_lib.T2S_FLAG_FORCED if is_forced[j] else (_lib.T2S_FLAG_IGNORE_EOS if ignore_eos else 0)) |
                 (_lib.T2S_FLAG_GUIDED if kinds[j] else 0) for j in range(n)]
        for j in range(n):         # the token row of a forced / prefixed dialogue holds its tokens before its first step
            if is_forced[j]:
                b["tokens"][text[j], :, :lim[j]].copy_(ops.h2d(forced[j], self.device))
            elif pre[j] is not None:
                b["tokens"][text[j], :, :pre[j].shape[1]].copy_(ops.h2d(pre[j], self.device))
        owner = [j for j in range(n) for _ in range(2 if kinds[j] else 1)]           # record -> utterance
        rows = settings_rows(resolved, [0 if p_ is None else p_.shape[1] for p_ in pre])
        b["per"][:nrec].copy_(ops.h2d(rows[torch.tensor(owner, dtype=torch.int64)].contiguous(), self.device))
        if ruled:
            b["rules"][:nrec].copy_(ops.h2d(rules_rows(rules)[torch.tensor(owner, dtype=torch.int64)].contiguous(), self.device))
        rec = torch.tensor([[ctx[r], lim[owner[r]], flags[owner[r]], 0, 0, 0, 0, 0] for r in range(nrec)], dtype=torch.int32)
        b["dialogues"][:nrec].copy_(rec)
        b["queue"].copy_(torch.tensor([0, nrec], dtype=torch.int32))
        b["state"].copy_(self._slot_records([]))
        self._run_steps(1.0, nb, 0, 1.0, True, None, nrec, scored, True, ng, ruled)  # the scheduler alone: arms the first slots
        return self._queue_chunks(lambda: self._run_chunk(1.0, nb, 1.0, True, None, nrec, scored, True, ng, ruled), nrec, text, lim, span, scored, on_done,
                                  lambda records: [list(records[text[j]]) + [records[text[j] + 1][5] if kinds[j] else None] for j in range(n)])

    # ------------------------------------------------------------------ beam search
    def _beam_scale(self, cond_scale) -> float:
        """check_beam_scale, and guidance is for one-output models (as in generate_batch)"""
        scale = check_beam_scale(cond_scale)
        if scale > 1.0 and self.d["streams"] != 1:
            raise NotImplementedError("guidance (cond_scale > 1) on a two-output model: the reference cannot run it (generate_batch)")
        return scale

    def _rule_bound(self, max_length) -> int:
        """the bound of min_length (check_rules): the steps the call may take; a call without steps is refused by its own check, not here"""
        return max(0, min(int(max_length or self.max_length), self.max_length))

    def _beam_rules(self, max_length, *rule_scalars) -> None:
        """A beam search WITHOUT the `beam_rules` switch takes no history rules: the scalars are validated (`check_rules`), and any rule
        switched on is a ValueError.  (With the switch: `check_beam_rules`, cvx_t2s_beam_rules_steps.)"""
        if rules_active(check_rules(None, 1, self._rule_bound(max_length), *rule_scalars)):
            raise ValueError("beam search does not run the history rules (repetition_penalty, no_repeat_ngram_size, min_length): a hypothesis' "
                             "history lives in the ancestry table - pass beam_rules=True (no_repeat_ngram_size, min_length), sample instead, or leave them off")

    def _ensure_beam(self) -> dict:
        """Device state of the beam chain (cvx_t2s_beam), for the decode buffers' current slot capacity: allocated on first use, and again
        when those buffers were re-allocated.  Nothing else holds its addresses but the beam graphs."""
        if getattr(self, "_beam", None) is not None and self._beam["gen"] == self._gen:
            return self._beam
        n, L, S, dev = self._slots, self.max_length, self.d["streams"], self.device
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self._beam = dict(gen=self._gen, scores=f32(n), finished=torch.zeros(n, dtype=torch.uint8, device=dev), owner=i32(2 * n * L),
                          groups=i32(n, 4), parents=i32(L * n), hist_tokens=i32(L * n * S), hist_logprobs=f32(L * n * S),
                          short_lp=f32(n * S * BEAM_MAX), short_tokens=i32(n * S * BEAM_MAX), logprobs=f32(n, S, L),
                          rules=i32(n, _lib.T2S_RULES_WORDS))     # (cvx_t2s_beam_rules_steps, lock-step: a row per group)
        return self._beam

    def _launch_beam(self, batch: int, beam_size: int, n: int, backtrack: bool = False, scale: float = 1.0, ruled: bool = False) -> None:
        """n steps of the beam chain (cvx_t2s_beam_steps) on the current stream; backtrack: then tokens / log-probs from the back-pointers.
        scale > 1: the guided chain (cvx_t2s_beam_guided_steps) - `batch` slots are batch / 2 hypotheses.  ruled: either chain under the
        rules table of the beam state, a row per group (cvx_t2s_beam_rules_steps)."""
        bm = self._ensure_beam()
        dec = self._descriptor(1.0, batch, scale)
        bs = _lib.T2SBeam(C.sizeof(_lib.T2SBeam), beam_size, self.max_length, 1 if backtrack else 0,
                          *[bm[k].data_ptr() for k in ("scores", "finished", "owner", "groups", "parents", "hist_tokens", "hist_logprobs",
                                                      "short_lp", "short_tokens", "logprobs")])
        if ruled:
            ru = _lib.T2SRules(C.sizeof(_lib.T2SRules), bm["rules"].shape[0], bm["rules"].data_ptr())
            _lib.check(_lib.load().cvx_t2s_beam_rules_steps(C.byref(dec), C.byref(bs), None, C.byref(ru), n, ops._stream()), "cvx_t2s_beam_rules_steps")
            return
        if scale > 1.0:
            _lib.check(_lib.load().cvx_t2s_beam_guided_steps(C.byref(dec), C.byref(bs), n, ops._stream()), "cvx_t2s_beam_guided_steps")
            return
        _lib.check(_lib.load().cvx_t2s_beam_steps(C.byref(dec), C.byref(bs), n, ops._stream()), "cvx_t2s_beam_steps")

    def _beam_idle(self) -> None:
        """every slot idle, every group ended: the state a warm-up or a capture may run on"""
        self.buf["state"].copy_(self._slot_records([]))
        g = torch.zeros(self._slots, 4, dtype=torch.int32)
        g[:, 1] = 1
        self._ensure_beam()["groups"].copy_(g)

    def _beam_graph(self, batch: int, beam_size: int, scale: float = 1.0, ruled: bool = False):
        """The captured graph of CHUNK beam steps for this (batch, beam size, stream CU count), through `_capture` as `_graph`'s, under a key of its own shape.
        The guided chain (scale > 1) has graphs of its own kind, "beamg", whose key carries the scale (a kernel argument).  ruled: the key
        gains a "rules" marker, not the values - the table is device memory, so one graph serves every mix of rules."""
        self._ensure_beam()
        key = ("beamg", beam_size, batch, float(scale), ops.stream_cus(), self._gen) if scale > 1.0 else \
            ("beam", beam_size, batch, ops.stream_cus(), self._gen)
        if ruled:
            key += ("rules",)
        return self._capture(key, lambda: self._launch_beam(batch, beam_size, CHUNK, scale=scale, ruled=ruled), self._beam_idle)

    def _beam_slot_records(self, ctx, B: int, nb: int, guided: bool) -> torch.Tensor:
        """slot records [slots, SR] (CPU) of nb beam slots at position 0, the others idle (`_slot_records`); ctx: context rows per dialogue
        row.  Unguided: the B hypotheses of utterance u are slots [u B, (u + 1) B) on dialogue row u; guided: 2 B slots, even ones on row
        2u (the text context), odd ones on row 2u + 1 (the null context) - the rows of `_guided_contexts`."""
        rec = self._slot_records([])
        rows = [2 * (i // (2 * B)) + (i & 1) if guided else i // B for i in range(nb)]
        rec[:nb] = torch.tensor([[0, 0, 0, ctx[r], r, 0, 0, 0] for r in rows], dtype=torch.int32)
        return rec

    def _beam_results(self, B: int, length_penalty: float, scores, lengths, tokens, logprobs, parents, h_tok, h_lp, steps, status=None) -> list:
        """Per utterance the list of its B hypotheses (flat tokens, streams, logprobs, score), best first (`beam_rank`), and its record in
        `last_beam`.  Per hypothesis u B + i (host): scores [n B], lengths (a list), tokens and logprobs [n B, S, L]; the search's history
        per utterance (device; the first steps[u] rows are copied): parents [n, L, B], h_tok and h_lp [n, L, B, S]; status: optional
        (status, group) per utterance."""
        S, out = self.d["streams"], []
        for u, T in enumerate(steps):
            ln, sc = lengths[u * B:(u + 1) * B], scores[u * B:(u + 1) * B]
            order = beam_rank(sc, ln, S, length_penalty)
            out.append([self._mask_after_eos(tokens[u * B + i, :, :ln[i]]) + (logprobs[u * B + i, :, :ln[i]].clone(), float(sc[i])) for i in order])
            self.last_beam.append(dict(steps=T, order=order, lengths=ln, scores=sc.clone(), parents=parents[u, :T].cpu(),
                                       tokens=h_tok[u, :T].cpu(), logprobs=h_lp[u, :T].cpu()))
            if status is not None:
                self.last_beam[-1].update(status=status[u][0], group=status[u][1])
        return out

    def _beam_wave(self, sources, B: int, max_len: int, length_penalty: float, scale: float = 1.0, rules=None) -> list:
        """One lock-step wave: utterance u in slots [u B, (u + 1) B).  -> per utterance the list of its B hypotheses, best first.
        scale > 1 (guided): hypothesis h is the slot pair (2h, 2h + 1) - text context / null context - and utterance u owns the kv_c rows
        2u (its context) and 2u + 1 (the null key / value alone), as in a guided generate_batch; everything kept per hypothesis (scores, history,
        back-tracked rows) has nh = n B rows, everything per slot nb = 2 nh.
        rules: None, or the n tuples of `check_beam_rules` - the wave runs under them (cvx_t2s_beam_rules_steps), utterance u by row u."""
        d = self.d
        S, n = d["streams"], len(sources)
        guided = scale > 1.0
        nh = n * B
        nb = 2 * nh if guided else nh
        self._ensure(nb, nb, 0)
        bm = self._ensure_beam()
        ruled = rules is not None
        graph = self._beam_graph(nb, B, scale, ruled) if os.environ.get("CVX_GRAPH", "1") == "1" else None
        if ruled:
            bm["rules"].zero_()
            bm["rules"][:n].copy_(ops.h2d(rules_rows(rules), self.device))
        ctx = self._guided_contexts(sources) if guided else self._contexts(sources)
        self.buf["state"].copy_(self._beam_slot_records(ctx, B, nb, guided))
        self.buf["x"][:nb].copy_(self.start[None, :].expand(nb, -1))
        sc = torch.full((self._slots,), -math.inf)
        sc[0:nh:B] = 0.0                                   # before step 0 only hypothesis 0 of an utterance is live
        bm["scores"].copy_(sc)
        bm["finished"].zero_()
        bm["owner"].copy_(torch.arange(self._slots, dtype=torch.int32)[None, :, None].expand(2, -1, self.max_length).reshape(-1))
        g = torch.zeros(self._slots, 4, dtype=torch.int32)
        g[:, 1] = 1
        g[:n, 1], g[:n, 2] = 0, max_len
        bm["groups"].copy_(g)
        self._chunks(graph.replay if graph is not None else lambda: self._launch_beam(nb, B, CHUNK, scale=scale, ruled=ruled), self.buf["state"], nb,
                     lambda st: all(r[1] for r in st), (max_len + CHUNK - 1) // CHUNK)
        self._launch_beam(nb, B, 0, backtrack=True, scale=scale)
        st = self._read_state(nb)[::2 if guided else 1]    # (per hypothesis: the text half's record)
        L = self.max_length                                # the history is kept per hypothesis: [steps, nh, ...]
        hist = lambda name, *tail: bm[name][:L * nh * math.prod(tail)].view(L, n, B, *tail).transpose(0, 1)
        scores, steps = bm["scores"][:nh].cpu(), [row[0] for row in bm["groups"][:n].tolist()]
        return self._beam_results(B, length_penalty, scores, [r[2] for r in st], self.buf["tokens"][:nh].cpu(), bm["logprobs"][:nh].cpu(),
                                  hist("parents"), hist("hist_tokens", S), hist("hist_logprobs", S), steps)

    @ops.gated
    @torch.no_grad()
    def generate_beam(self, sources, beam_size: int = 10, max_length: Optional[int] = None, length_penalty: float = 1.0,
                      return_beams: bool = False, cond_scale: float = 1.0, repetition_penalty: float = 1.0, repetition_window: int = 0,
                      no_repeat_ngram_size=0, min_length=0, beam_rules: bool = False):
        """Beam search (the algorithm: include/covomix_hip.h, cvx_t2s_beam_steps): deterministic, no draws - temperature, logit filter and
        uniforms play no part.  Every step keeps the beam_size hypotheses with the largest cumulative log-probability (fp32); a hypothesis
        that takes an eos in any stream is finished and competes with its score unchanged; the utterance ends when all are finished or after
        max_length steps.  The hypotheses of an utterance sit in beam_size neighbouring decode slots and continue from each other's KV
        caches through a device-side ancestry table - no cache row is copied.
        sources: one text ([n] / [1, n] ids) or a list; a list runs in lock-step waves of MAX_BATCH // beam_size utterances (each ends on
        its own, its slots then idle).  beam_size: 1..16 (the reference's default is 10).
        Returns, per utterance, (flat tokens, streams int64 [S, L], logprobs float32 [S, L], score) of the hypothesis with the largest
        score / (L * S) ** length_penalty (ties: the lowest slot) - host tensors; score is the cumulative log-probability, the fp32 sum
        the selection kept, and logprobs equal, bit for bit, what score_many gives for `streams`.  return_beams: the list of all beam_size
        hypotheses instead, best first (dead ones, score -inf, last).  `last_beam` keeps, per utterance of the call, the records of the search
        (tests, tools): steps, the slots best first (`order`), their lengths and scores, and the back-pointers parents [steps, B], tokens /
        logprobs [steps, B, S] (beam_backtrack turns them into sequences).
        cond_scale > 1 (one-output models): beam search under classifier-free guidance (cvx_t2s_beam_guided_steps) - every hypothesis is a
        slot pair (text context, null context), the search ranks by the log-softmax of null + (cond - null) * cond_scale, and logprobs
        equal, bit for bit, score_many(..., cond_scale=cond_scale); waves hold MAX_BATCH // (2 * beam_size) utterances.  Return values and
        `last_beam` have the same shape.  ValueError for cond_scale < 1, NotImplementedError for a two-output model.
        Without beam_rules the history rules (generate_batch) do not run under beam search: any of them switched on is a ValueError
        (`_beam_rules`).  beam_rules=True: no_repeat_ngram_size and min_length - each a scalar or one value per utterance
        (`check_beam_rules`) - remove candidates along every hypothesis' own ancestry (cvx_t2s_beam_rules_steps: the bans act on the
        log-softmax, so scores and logprobs stay the model's and still equal score_many bit for bit); with both off for everyone the plain
        chain runs.  A repetition_penalty other than 1 stays a ValueError."""
        one = torch.is_tensor(sources)
        srcs = [sources] if one else list(sources)
        rules = None
        if beam_rules:
            rules = check_beam_rules(len(srcs), self._rule_bound(max_length), repetition_penalty, repetition_window, no_repeat_ngram_size, min_length)
            rules = rules if rules_active(rules) else None
        else:
            self._beam_rules(max_length, repetition_penalty, repetition_window, no_repeat_ngram_size, min_length)
        B = check_beam_size(beam_size)
        scale = self._beam_scale(cond_scale)
        max_len = min(int(max_length or self.max_length), self.max_length)
        if max_len < 1:
            raise ValueError("generate_beam needs at least one step")
        self.last_beam = []
        per, out = MAX_BATCH // (2 * B if scale > 1.0 else B), []
        for w in range(0, len(srcs), per):
            out += self._beam_wave(srcs[w:w + per], B, max_len, float(length_penalty), scale, rules[w:w + per] if rules else None)
        res = out if return_beams else [h[0] for h in out]
        return res[0] if one else res

    # ------------------------------------------------------------------ beam search through continuously refilled groups
    def _ensure_beam_queue(self, records: int) -> dict:
        """Device state of cvx_t2s_beam_queue for `records` hypotheses (utterances * beam_size) queued at a time: allocated on first use, and
        again when it must grow or the decode buffers were re-allocated.  The ancestry table of this chain is its own and gets its values
        here, on the device, once.  Only the "beamq" graphs hold these addresses: they are dropped with the buffers."""
        bq = getattr(self, "_beamq", None)
        if bq is not None and bq["gen"] == self._gen and bq["records"] >= records:
            return bq
        for key in [k for k in self._graphs if k[0] in ("beamq", "beamqg")]:
            del self._graphs[key]
        R, n, L, S, dev = max(records, 8), self._slots, self.max_length, self.d["streams"], self.device
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self._beamq = dict(gen=self._gen, records=R, queue=i32(2), utterances=i32(R, SR), parents=i32(R * L), hist_tokens=i32(R * L * S),
                           hist_logprobs=f32(R * L * S), final_scores=f32(R), final_steps=i32(R),
                           final_finished=torch.zeros(R, dtype=torch.uint8, device=dev),
                           tokens=torch.zeros(R, S, L, dtype=torch.int64, device=dev), logprobs=f32(R, S, L),
                           rules=i32(R, _lib.T2S_RULES_WORDS),   # (cvx_t2s_beam_rules_steps, queue form: a row per utterance)
                           owner=torch.arange(n, dtype=torch.int32, device=dev)[None, :, None].expand(2, -1, L).contiguous(),
                           slot_ids=torch.arange(n, dtype=torch.int32, device=dev))
        return self._beamq

    def _launch_beam_queue(self, batch: int, beam_size: int, n_utt: int, n: int, backtrack: bool = False, scale: float = 1.0,
                           ruled: bool = False) -> None:
        """n steps of the refilled beam chain (cvx_t2s_beam_queue_steps) on the current stream; backtrack: then tokens / log-probs of every
        (utterance, hypothesis) from the per-utterance back-pointers.  scale > 1: cvx_t2s_beam_guided_queue_steps.  ruled: either under
        the rules table of the queue state, a row per utterance (cvx_t2s_beam_rules_steps)."""
        bm, bq = self._ensure_beam(), self._beamq
        dec = self._descriptor(1.0, batch, scale)
        bs = _lib.T2SBeam(C.sizeof(_lib.T2SBeam), beam_size, self.max_length, 1 if backtrack else 0, bm["scores"].data_ptr(),
                          bm["finished"].data_ptr(), bq["owner"].data_ptr(),
                          *[bm[k].data_ptr() for k in ("groups", "parents", "hist_tokens", "hist_logprobs", "short_lp", "short_tokens", "logprobs")])
        qs = _lib.T2SBeamQueue(C.sizeof(_lib.T2SBeamQueue), n_utt, bq["queue"].data_ptr(), bq["utterances"].data_ptr(), self.start.data_ptr(),
                               *[bq[k].data_ptr() for k in ("parents", "hist_tokens", "hist_logprobs", "final_scores", "final_steps",
                                                           "final_finished", "tokens", "logprobs")])
        if ruled:
            ru = _lib.T2SRules(C.sizeof(_lib.T2SRules), bq["rules"].shape[0], bq["rules"].data_ptr())
            _lib.check(_lib.load().cvx_t2s_beam_rules_steps(C.byref(dec), C.byref(bs), C.byref(qs), C.byref(ru), n, ops._stream()),
                       "cvx_t2s_beam_rules_steps")
            return
        if scale > 1.0:
            _lib.check(_lib.load().cvx_t2s_beam_guided_queue_steps(C.byref(dec), C.byref(bs), C.byref(qs), n, ops._stream()),
                       "cvx_t2s_beam_guided_queue_steps")
            return
        _lib.check(_lib.load().cvx_t2s_beam_queue_steps(C.byref(dec), C.byref(bs), C.byref(qs), n, ops._stream()), "cvx_t2s_beam_queue_steps")

    def _beam_queue_graph(self, batch: int, beam_size: int, scale: float = 1.0, ruled: bool = False):
        """The captured graph of CHUNK steps of the refilled beam chain (`_capture`).  (The number of utterances sizes the
        back-track launch only, which is not part of the graph: the steps read the device-side queue.)  Guided: kind "beamqg", with the scale."""
        key = ("beamqg", beam_size, batch, float(scale), ops.stream_cus(), self._gen) if scale > 1.0 else \
            ("beamq", beam_size, batch, ops.stream_cus(), self._gen)
        if ruled:                                          # (a marker, not the values: one graph serves every mix)
            key += ("rules",)
        return self._capture(key, lambda: self._launch_beam_queue(batch, beam_size, 1, CHUNK, scale=scale, ruled=ruled), self._beam_idle)

    def _beam_queue_window(self, sources, B: int, lim: list, length_penalty: float, slots: int, scale: float = 1.0, rules=None) -> list:
        """One window of generate_beam_many: its utterances' contexts resident, the groups refilled on the device until all have ended.
        scale > 1 (guided): a group is 2 B slots - the pairs of _beam_wave - and utterance j owns the kv_c rows 2j and 2j + 1."""
        d = self.d
        S, n, L = d["streams"], len(sources), self.max_length
        guided = scale > 1.0
        P = 2 if guided else 1                             # slots per hypothesis
        G = max(1, min(slots // (P * B), MAX_BATCH // (P * B), n))
        nb = G * B * P                                     # (the buffers hold whole 8-slot kernel groups: _ensure)
        self._ensure(nb, n * P, 0)
        bm, bq = self._ensure_beam(), self._ensure_beam_queue(max(n * B, WINDOW))
        ruled = rules is not None                          # (the n tuples of check_beam_rules: utterance j by row j)
        graph = self._beam_queue_graph(nb, B, scale, ruled) if os.environ.get("CVX_GRAPH", "1") == "1" else None
        if ruled:
            bq["rules"].zero_()
            bq["rules"][:n].copy_(ops.h2d(rules_rows(rules), self.device))
        ctx = self._guided_contexts(sources) if guided else self._contexts(sources)
        self.buf["state"].copy_(self._beam_slot_records(ctx, B, nb, guided))
        self.buf["x"][:nb].copy_(self.start[None, :].expand(nb, -1))
        sc = torch.full((self._slots,), -math.inf)
        sc[0:G * B:B] = 0.0                                # before step 0 only hypothesis 0 of an utterance is live
        bm["scores"].copy_(sc)
        bm["finished"].zero_()
        g = torch.zeros(self._slots, 4, dtype=torch.int32)
        g[:, 1] = 1
        for u in range(G):                                 # group u starts on utterance u
            g[u] = torch.tensor([0, 0, lim[u], u], dtype=torch.int32)
        bm["groups"].copy_(g)
        bq["owner"].view(2, self._slots, L)[0, :nb, 0].copy_(bq["slot_ids"][:nb])     # (position 0 of a starting slot: the slot itself)
        bq["utterances"][:n].copy_(torch.tensor([[ctx[P * j], lim[j], 0, 1 if j < G else 0, 0, j if j < G else 0, 0, 0] for j in range(n)],
                                                dtype=torch.int32))
        bq["queue"].copy_(torch.tensor([G, n], dtype=torch.int32))
        done = lambda r: all(row[3] >= 2 for row in r)
        cap = (sum(lim) + CHUNK - 1) // CHUNK + 4          # (one group decoding everything: cannot be reached)
        i, rec = self._chunks(graph.replay if graph is not None else lambda: self._launch_beam_queue(nb, B, n, CHUNK, scale=scale, ruled=ruled), bq["utterances"], n, done, cap)
        if not done(rec):
            raise RuntimeError(f"text2semantic refilled beam decode: {sum(1 for row in rec if row[3] < 2)} of {n} utterances did not finish in {i} chunks")
        self._launch_beam_queue(nb, B, n, 0, backtrack=True, scale=scale)
        hist = lambda name, *tail: bq[name][:n * L * B * math.prod(tail)].view(n, L, B, *tail)
        return self._beam_results(B, length_penalty, bq["final_scores"][:n * B].cpu(), bq["final_steps"][:n * B].tolist(), bq["tokens"][:n * B].cpu(),
                                  bq["logprobs"][:n * B].cpu(), hist("parents"), hist("hist_tokens", S), hist("hist_logprobs", S),
                                  [row[4] for row in rec], [(row[3], row[5]) for row in rec])

    @ops.gated
    @torch.no_grad()
    def generate_beam_many(self, sources, beam_size: int = 10, max_length: Optional[int] = None, length_penalty: float = 1.0,
                           return_beams: bool = False, slots: int = 64, limits=None, cond_scale: float = 1.0, repetition_penalty: float = 1.0,
                           repetition_window: int = 0, no_repeat_ngram_size=0, min_length=0, beam_rules: bool = False):
        """generate_beam for ANY number of utterances through continuously refilled slot GROUPS (cvx_t2s_beam_queue_steps): slots // beam_size
        groups (at most MAX_BATCH // beam_size) of beam_size neighbouring slots; a group whose utterance has ended - all hypotheses finished,
        or its step limit - takes the next pending utterance inside the selection kernel of that very step, as generate_many's slots do.
        Every utterance gets, bit for bit, what generate_beam gives it alone.  limits: optional per-utterance step limits (default
        max_length for all).  Windows of WINDOW // beam_size utterances (a record is a hypothesis), one packed encoder pass each.
        Returns what generate_beam returns for a list, in input order, host tensors; `last_beam` keeps generate_beam's record per utterance
        plus `status` (2: all hypotheses finished, 3: step limit) and `group` (the group it ran in).
        cond_scale > 1 (one-output models): the guided search of generate_beam(cond_scale=...) through slots // (2 * beam_size) groups of
        slot pairs (cvx_t2s_beam_guided_queue_steps); every utterance again equals generate_beam(cond_scale=...) alone, bit for bit.
        ValueError (before any device work): beam_size outside 1..16, slots that hold no group (slots < beam_size, or < 2 * beam_size under
        guidance), cond_scale < 1, limits of another length than sources, any history rule switched on without beam_rules (`_beam_rules`).
        NotImplementedError: guidance on a two-output model.
        beam_rules=True: no_repeat_ngram_size / min_length as in generate_beam, a scalar or one value per utterance; an utterance's history
        is its own ancestry, so a refilled group is not affected by its predecessor, and every utterance equals generate_beam alone with its
        own values, bit for bit."""
        srcs = list(sources)
        n = len(srcs)
        rules = None
        if beam_rules:
            rules = check_beam_rules(n, self._rule_bound(max_length), repetition_penalty, repetition_window, no_repeat_ngram_size, min_length)
            rules = rules if rules_active(rules) else None
        else:
            self._beam_rules(max_length, repetition_penalty, repetition_window, no_repeat_ngram_size, min_length)
        B = check_beam_size(beam_size)
        scale = self._beam_scale(cond_scale)
        if int(slots) < (2 * B if scale > 1.0 else B):
            raise ValueError(f"generate_beam_many: slots = {slots} hold no {'guided ' if scale > 1.0 else ''}group of beam_size = {B}")
        if limits is not None and len(limits) != n:
            raise ValueError(f"generate_beam_many: {len(limits)} limits for {n} utterances")
        max_len = min(int(max_length or self.max_length), self.max_length)
        if max_len < 1:
            raise ValueError("generate_beam_many needs at least one step")
        lim = [max_len] * n if limits is None else [max(1, min(int(x), max_len)) for x in limits]
        self.last_beam = []
        out, win = [], max(1, WINDOW // B)
        for w in range(0, n, win):
            out += self._beam_queue_window(srcs[w:w + win], B, lim[w:w + win], float(length_penalty), int(slots), scale,
                                           rules[w:w + win] if rules else None)
        return out if return_beams else [h[0] for h in out]

    # ------------------------------------------------------------------ prefill: one causal full-sequence pass over given tokens
    def _prefill_check(self) -> None:
        """The widths the full-sequence kernels admit: the fp32 GEMM reads rows in 16-byte pieces (K, lda % 4 == 0), and the logits GEMM of
        stream s starts at column s * dim_emb of the normed rows.  ValueError otherwise - the step chain takes any width."""
        d = self.d
        if d["dim_target"] % 4 or d["dim_emb"] % 4:
            raise ValueError(f"prefill=True: the full-sequence GEMMs need dim_target ({d['dim_target']}) and the semantic embedding width "
                             f"({d['dim_emb']}) to be multiples of 4; run this model without prefill")

    def _prefill(self, seqs, nulls=None, scales=None, cache: bool = False, return_logits: bool = False):
        """ONE pass of the target transformer over the packed rows of `seqs` (`prefill_rows`: (tokens [S, L], record, ctx, slot) each; the
        kv_c rows of the records are in place - `_contexts`), layer by layer in the decode's order on the full-sequence kernels: RMSNorm,
        the fp32 GEMMs (to_qkv with the RoPE epilogue at every row's position), GEGLU, and the two attentions on
        ops.t2s_prefill_attention - causal over the pass' own q | k | v rows, then over [0, ctx) of the record's kv_c.
        nulls / scales (guidance): the first len(nulls) sequences are the ones scored; nulls[j] >= 0 names the sequence that ran the same
        tokens with ctx = 1, and the scored rows become null + (cond - null) * scales[j] (ops.t2s_prefill_guidance); -1: unguided.
        Default: every sequence is scored as it is.  cache: the rotated keys and the values of every layer go into k_cache / v_cache of
        the sequences' slots, positions 0 .. L - 1.
        -> per scored sequence the log-probs float32 [S, L] of its tokens (cvx_t2s_logprob_f32: the decode's summation order) on the
        device; with return_logits (tests) also its logits [L, S, V], the rows the log-probs were taken from."""
        self._prefill_check()
        d, dev = self.d, self.device
        S, V, I, H, D, E, F_ = d["streams"], d["vocab"], d["inner"], d["heads"], d["dim_target"], d["dim_emb"], d["ff_tgt"]
        t = prefill_rows(seqs, S, self.max_length, self.max_source + 2)
        M, n, cu_host = t["rows"], len(seqs), t["cu"].tolist()
        n_out = n if nulls is None else len(nulls)
        Mc = cu_host[n_out]
        if cache and max(s_[3] for s_ in seqs) >= self._slots:
            raise ValueError("prefill: a cache slot beyond the decode buffers")
        cu, kbase, nk = (ops.h2d(t[k], dev) for k in ("cu", "kbase", "nk"))
        pos, starts = ops.h2d(t["positions"], dev), ops.h2d(t["starts"], dev)
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        x = self.emb.index_select(0, ops.h2d(t["gather"].reshape(-1), dev)).view(M, D)
        x.index_copy_(0, starts, self.start[None, :].expand(n, -1))
        rope = (self.rope[0].index_select(0, pos), self.rope[1].index_select(0, pos))        # per-row tables (rope_T = M)
        normed, qkv, att, qc, h2, hg = f(M, D), f(M, 3 * I), f(M, I), f(M, I), f(M, 2 * F_), f(M, self.Fp)
        dst = ops.h2d(t["cache"], dev) if cache else None
        scale = 64 ** -0.5
        for L in self.dec:
            ops.adarmsnorm(x, L["gamma_s"], None, normed)
            ops.gemm(normed, L["wqkv_s"], qkv, rope=rope, rope_cols=2 * I)
            ops.t2s_prefill_attention(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], att, cu, cu, None, t["max_q"], H, scale, True)
            if cache:
                L["k_cache"].view(-1, I).index_copy_(0, dst, qkv[:, I:2 * I])
                L["v_cache"].view(-1, I).index_copy_(0, dst, qkv[:, 2 * I:])
            ops.gemm(att, L["wo_s"], x, residual=x)
            ops.adarmsnorm(x, L["gamma_c"], None, normed)
            ops.gemm(normed, L["wq_c"], qc)
            kv = L["kv_c"].view(-1, 2 * I)
            ops.t2s_prefill_attention(qc, kv[:, :I], kv[:, I:], att, cu, kbase, nk, t["max_q"], H, scale, False)
            ops.gemm(att, L["wo_c"], x, residual=x)
            ops.adarmsnorm(x, L["gamma_f"], None, normed)
            ops.gemm(normed, L["w1"], h2, bias=L["b1"])
            ops.geglu(h2, hg, F_)
            ops.gemm(hg, L["w2"], x, bias=L["b2"], residual=x)
        ops.adarmsnorm(x, self.dec_final, None, normed)
        logits = f(M, S, V)
        for s_ in range(S):
            ops.gemm(normed[:, s_ * E:(s_ + 1) * E], self.emb, logits[:, s_, :])
        if nulls is not None and any(k >= 0 for k in nulls):                                 # (guidance: one-output models, S = 1)
            null_row = torch.full((Mc,), -1, dtype=torch.int32)
            row_scale = torch.ones(Mc, dtype=torch.float32)
            for j, k in enumerate(nulls):
                if k >= 0:
                    null_row[cu_host[j]:cu_host[j + 1]] = torch.arange(cu_host[k], cu_host[k + 1], dtype=torch.int32)
                    row_scale[cu_host[j]:cu_host[j + 1]] = float(scales[j])
            ops.t2s_prefill_guidance(logits.view(M * S, V), ops.h2d(null_row, dev), ops.h2d(row_scale, dev))
        lp = ops.t2s_logprob(logits[:Mc].view(Mc * S, V), ops.h2d(t["targets"][:Mc].reshape(-1), dev)).view(Mc, S)
        out = [lp[cu_host[j]:cu_host[j + 1]].T.contiguous() for j in range(n_out)]
        if return_logits:
            return out, [logits[cu_host[j]:cu_host[j + 1]] for j in range(n_out)]
        return out

    def _prefill_pairs(self, tokens, text, ctx_text, scales, slots: bool):
        """The sequences of a pass over `tokens` (int64 [S, L] each; utterance j sits in record text[j] with ctx_text[j] context rows, the
        null half of a guided one - scales[j] > 1 - in record text[j] + 1): the text halves first, then the null halves.
        slots: every record's caches are those of the slot of the same number.  -> (seqs, nulls) for `_prefill`."""
        seqs = [(tokens[j], text[j], ctx_text[j], text[j] if slots else None) for j in range(len(tokens))]
        nulls = [-1] * len(tokens)
        for j in range(len(tokens)):
            if scales[j] > 1.0:
                nulls[j] = len(seqs)
                seqs.append((tokens[j], text[j] + 1, 1, text[j] + 1 if slots else None))
        return seqs, nulls

    @ops.gated
    @torch.no_grad()
    def _score_prefill(self, sources, tg, scales, return_logits: bool = False):
        """score_many(prefill=True): windows of at most PREFILL_ROWS packed rows and WINDOW dialogue records, each one encoder pass
        (`_contexts` into the records of `mixed_records`) and one `_prefill` pass.  No decode slot, no queue, no graph."""
        self._prefill_check()
        kinds = [c > 1.0 for c in scales]
        out, lgs = [], []
        for w0, w1 in prefill_windows([t.shape[1] * (2 if g else 1) for t, g in zip(tg, kinds)], PREFILL_ROWS, [2 if g else 1 for g in kinds]):
            first = mixed_records(kinds[w0:w1])
            text = first[:-1]
            self._ensure(0, first[-1], 0)
            ctx_text = self._contexts(sources[w0:w1], text)
            nulls = [text[j] + 1 for j in range(w1 - w0) if kinds[w0 + j]]
            if nulls:              # the null half: the learned null key / value row only
                ni = ops.h2d(torch.tensor(nulls, dtype=torch.int64), self.device)
                for L in self.dec:
                    L["kv_c"][:, 0].index_copy_(0, ni, L["null"][None, :].expand(len(nulls), -1))
            seqs, null_of = self._prefill_pairs(tg[w0:w1], text, ctx_text, scales[w0:w1], False)
            res = self._prefill(seqs, null_of, scales[w0:w1], return_logits=return_logits)
            if return_logits:
                lgs += [x.cpu() for x in res[1]]
                res = res[0]
            out += [x.cpu() for x in res]
        return (out, lgs) if return_logits else out

    def score_many(self, sources, targets, cond_scale=1.0, slots: int = 64, mixed_guidance: bool = False, prefill: bool = False):
        """Teacher-forced scoring: the log-probability the model gives every token of targets[j] under the text sources[j] - what the
        reference's TextToSemantic.forward(..., return_loss=True) averages (text2semantic.py), position by position.  targets[j]: int64
        [S, L_j], the `streams` that `generate` returns; -> list of float32 [S, L_j] host tensors: entry [s, t] is the log-softmax, at
        token targets[j][s, t], of the step-t logits given the tokens before t (the guidance-combined logits under cond_scale > 1, one-output
        models).  The targets run as forced dialogues through `slots` continuously refilled decode slots, in windows of WINDOW records as
        generate_many; the values are bit-identical whatever the slots, the batch or the neighbours - and equal, bit for bit, the log-probs
        `generate(return_logprobs=True)` returned when it sampled those tokens.  ValueError for L_j < 1, L_j > max_length or a token
        outside [0, vocab); NotImplementedError for guidance on a two-output model.
        mixed_guidance: cond_scale may be a list, one scale per utterance - 1 (unguided) or > 1 (guided) - and all of them are scored in
        one generate_many(mixed_guidance=True) call.
        prefill (default False: the call as above): the log-probs come from causal full-sequence PASSES over the targets (`_prefill`;
        include/covomix_hip.h, cvx_t2s_prefill_attention_f32) instead of one decode step per token - no decode slot, no queue, no graph;
        `slots` is not looked at.  Same return type and shapes; cond_scale > 1 and mixed_guidance as above (a guided utterance is two
        sequences of a pass).  The values are fp32-class and inside the oracle bound of the step chain, but NOT bit-identical to it (a GEMM
        and a GEMV round differently), and an utterance's bits may depend on how many rows its pass holds; the
        same call twice gives the same bits.  ValueError for a model whose widths the full-sequence kernels do not admit
        (`_prefill_check`)."""
        sources, targets = list(sources), list(targets)
        if len(sources) != len(targets):
            raise ValueError(f"score_many: {len(sources)} sources, {len(targets)} targets")
        if mixed_guidance:
            scales = [float(c) for c in cond_scale] if isinstance(cond_scale, (list, tuple)) else [float(cond_scale)] * len(sources)
            if len(scales) != len(sources):
                raise ValueError(f"score_many: {len(scales)} cond_scale values for {len(sources)} utterances")
            check_settings([{"cond_scale": c} for c in scales], len(scales), self.d["vocab"], self.d["streams"], mixed=True)
            tg = check_targets(targets, self.d["streams"], self.d["vocab"], self.max_length)
            if not tg:
                return []
            if prefill:
                return self._score_prefill(sources, tg, scales)
            res = self.generate_many(sources, None, max(t.shape[1] for t in tg), 1.0, None, slots, return_logprobs=True, forced=tg,
                                     settings=[{"cond_scale": c} for c in scales], mixed_guidance=True)
            return [r[2] for r in res]
        if float(cond_scale) > 1.0 and self.d["streams"] != 1:
            raise NotImplementedError("guidance (cond_scale > 1) on a two-output model: the reference cannot run it (generate_batch)")
        tg = check_targets(targets, self.d["streams"], self.d["vocab"], self.max_length)
        if not tg:
            return []
        if prefill:
            return self._score_prefill(sources, tg, [float(cond_scale)] * len(tg))
        res = self.generate_many(sources, None, max(t.shape[1] for t in tg), 1.0, None, slots, cond_scale=cond_scale,
                                 return_logprobs=True, forced=tg)
        return [r[2] for r in res]

    @ops.gated
    def generate(self, source_ids: torch.Tensor, uniforms: Optional[torch.Tensor] = None, max_length: Optional[int] = None,
                 temperature: float = 1.0, generator: Optional[torch.Generator] = None, return_streams: bool = False,
                 collect_logits: bool = False, cond_scale: float = 1.0, filter_logits_fn="top_k", filter_fn_kwargs=None,
                 return_logprobs: bool = False, repetition_penalty: float = 1.0, repetition_window: int = 0, no_repeat_ngram_size: int = 0,
                 min_length: int = 0):
        """== TextToSemanticWrapper.sample(grapheme_token_ids): flat int64 tensor, stream 1 then stream 2 (two-output
        models), each cut after its eos.  uniforms [steps, streams, vocab] (or [steps, streams, 1, vocab]) replaces
        the random draws of gumbel_noise (text2semantic.py:108-110); default: torch.rand from `generator`.
        collect_logits (tests): step one token at a time without a graph and also return the pre-filter logits
        [steps, streams, vocab].  cond_scale / filter_logits_fn / filter_fn_kwargs: see generate_batch.  return_logprobs: returns
        (flat tokens, streams[, logits], logprobs) - logprobs float32 [S, length] aligned with streams (generate_batch).
        repetition_penalty / repetition_window / no_repeat_ngram_size / min_length: the history rules (generate_batch)."""
        if source_ids.ndim == 2 and source_ids.shape[0] != 1:
            raise NotImplementedError("one utterance per call (the generation scripts run batch 1); see generate_batch")
        res = self.generate_batch([source_ids], None if uniforms is None else [uniforms], max_length, temperature, generator,
                                  collect_logits, cond_scale, False, filter_logits_fn, filter_fn_kwargs, return_logprobs, repetition_penalty,
                                  repetition_window, no_repeat_ngram_size, min_length)[0]
        if collect_logits or return_logprobs:
            return res
        return res if return_streams else res[0]
