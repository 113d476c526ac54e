"""Shared by tests/test_t2s_beam_guided.py (CPU) and tests/test_t2s_beam_guided_gpu.py: the beam search under classifier-free guidance of
include/covomix_hip.h (cvx_t2s_beam_guided_steps) on the fp64 oracle - tests/t2s_beam_restated.py's oracle_beam with the guidance-combined
logits g = null + (cond - null) * scale (oracle/t2s_oracle.py teacher_forced_logits(cond_scale=scale)), the same candidates, margins and
records, and the unguided logit bound pushed through the combination.

Per-step bound: the combined row's error is at most scale * e_cond + (scale - 1) * e_null (g = scale * cond - (scale - 1) * null), and each
row's error is bounded as in the unguided search by 2 LONG_LOGIT_TOL times its norm, so
    2 LONG_LOGIT_TOL (scale ||cond||_2 + (scale - 1) ||null||_2) + LOGP_TOL_ULPS 2^-24 (1 + |lp|),
|lp| over the shortlists.  At scale = 1 this is oracle_beam's bound.  decidable_prefix of t2s_beam_restated is used as it is."""
import math

import torch

import t2s_beam_restated as br
import t2s_logprob_restated as rs

NEG = br.NEG
_CACHE: dict = {}


def oracle_beam_guided(sd, src, B, max_len, scale):
    """oracle_beam under guidance: -> list over steps of dict(hyps: list of B (prefix, score, finished, parent), margin, bound, ended)"""
    import t2s_oracle as orc
    d = orc.t2s_dims(sd)
    S = 2 if d["two_output"] else 1
    V = sd["semantic_token_emb.weight"].shape[0]
    scale = float(scale)
    no_text = torch.zeros(src.numel() + 1)                 # every text key masked out: the learned null key / value alone
    hyps = [((), 0.0 if i == 0 else NEG, False, 0) for i in range(B)]
    out = []
    for t in range(max_len):
        lp = torch.zeros(B, S, V, dtype=torch.float64)
        bound = 0.0
        for p, (pre, c, fin, _) in enumerate(hyps):
            if fin or not c > NEG:
                continue
            st = torch.tensor([list(x) for x in pre] + [[0] * S], dtype=torch.int64).T.reshape(S, -1)      # [S, t + 1]: the last entry is not read
            lg = orc.teacher_forced_logits(sd, src, st, cond_scale=scale, dtype=torch.float64)[-1]         # [S, V], combined
            cond = orc.teacher_forced_logits(sd, src, st, dtype=torch.float64)[-1]
            norm = scale * cond.norm(dim=-1)
            if scale > 1.0:
                null = orc.teacher_forced_logits(sd, src, st, dtype=torch.float64, context_mask=no_text)[-1]
                norm = norm + (scale - 1.0) * null.norm(dim=-1)
            lp[p] = torch.log_softmax(lg, dim=-1)
            top = lp[p].topk(min(B + 1, V), dim=-1).values
            per = 2 * orc.LONG_LOGIT_TOL * norm + rs.LOGP_TOL_ULPS * rs.EPS * (1.0 + top.abs().max(dim=-1).values)
            bound = max(bound, S * float(per.max()))
        sc = torch.tensor([h[1] for h in hyps], dtype=torch.float64)
        fin = torch.tensor([h[2] for h in hyps])
        cand = br.candidates(lp, sc, fin, B, extra=1)
        margin = float(cand[B - 1][0]) - float(cand[B][0]) if len(cand) > B else math.inf
        new = []
        for i in range(B):
            if i >= len(cand):
                new.append(((), NEG, True, i))
                continue
            score, q, p, toks, _ = cand[i]
            if toks is None:
                new.append((hyps[p][0], float(score), True, p))
            else:
                new.append((hyps[p][0] + (tuple(toks),), float(score), (V - 1) in toks, p))
        hyps = new
        ended = all(h[2] for h in hyps)
        out.append(dict(hyps=hyps, margin=margin, bound=bound, ended=ended))
        if ended:
            break
    return out


# the oracle cases of the CPU and the GPU test: (ids of the golden cosingle_small text, beam size, scale)
ORACLE_CASES = [(12, 3, 1.5), (12, 4, 1.5), (9, 2, 2.0)]
MAX_LEN = 40


def oracle_case(sd, src_full, ids, B, scale):
    """(steps, decidable prefix, accumulated bounds, re-parenting steps inside the prefix) of one case, computed once per process"""
    key = (ids, B, scale)
    if key not in _CACHE:
        steps = oracle_beam_guided(sd, src_full[:, :ids], B, MAX_LEN, scale)
        n, acc = br.decidable_prefix(steps)
        moved = sum(1 for s in steps[:n] if any(h[3] != i for i, h in enumerate(s["hyps"])))
        _CACHE[key] = (steps, n, acc, moved)
    return _CACHE[key]


# finished hypotheses: the eos embedding row = alpha * row EOS_LIKE, the token the guided greedy decode repeats
EOS_LIKE = 127
FINISHED_CASES = [(1.05, 3, 1.5), (0.95, 4, 1.5)]


def with_eos_row(sd, alpha):
    sd = dict(sd)
    E = sd["semantic_token_emb.weight"].clone()
    E[-1] = alpha * E[EOS_LIKE]
    sd["semantic_token_emb.weight"] = E
    return sd


def first_finish(steps):
    """prefix -> the step at which that hypothesis finished"""
    first = {}
    for t, s in enumerate(steps):
        for h in s["hyps"]:
            if h[2] and h[1] > NEG:
                first.setdefault(h[0], t)
    return first
