"""Shared by tests/test_t2s_beam.py (CPU) and tests/test_t2s_beam_gpu.py: the beam search of include/covomix_hip.h (cvx_t2s_beam_steps)
restated in torch on the CPU - the selection step in fp64 and in fp32, crafted blocks it is checked on, the back-tracking of its records, and
the whole search on the fp64 oracle (oracle/t2s_oracle.py teacher_forced_logits, one causal pass per live hypothesis and step).

Selection (per group of B hypotheses; S streams, V entries, eos = V - 1): lp = log_softmax per row; per live hypothesis and stream the
min(B, V) entries with the largest lp by (lp descending, index ascending); candidates (p, a[, b]) scored c[p] + lp0 or c[p] + (lp0 + lp1) with
key q = (p B + a) B + b; a finished p: itself, q = p B B; a p with c = -inf: none; the B best by (score descending, q ascending); a slot
without a candidate: dead (parent = itself, tokens -1, score -inf, finished)."""
import math

import torch

import t2s_logprob_restated as rs

NEG = -math.inf
GAP = 1e-3                     # crafted blocks: two candidates tie exactly or differ by more than this (fp64)


def _lp(logits, dtype):
    """log_softmax of every row: fp64 exactly, fp32 in the kernel's order of operations (t2s_logprob_restated)"""
    if dtype == torch.float64:
        return torch.log_softmax(logits.double(), dim=-1)
    l = logits.to(torch.float32)
    m = l.max(dim=-1, keepdim=True).values
    ex = torch.exp(l - m)
    s = rs.SUMS["kernel order"](ex.reshape(-1, ex.shape[-1])).reshape(ex.shape[:-1])
    return (l - m) - torch.log(s)[..., None]


def candidates(lp, scores, finished, B, extra=0):
    """One group.  lp [B, S, V] (any float dtype), scores [B], finished [B] -> list of (score, q, p, toks, lps) of every candidate; the
    shortlists hold min(B + extra, V) entries (extra = 1: the best REJECTED candidate of the search is among them too)."""
    S, V = lp.shape[1], lp.shape[2]
    K = min(B + extra, V)
    out = []
    for p in range(B):
        c = scores[p]
        if not float(c) > NEG:
            continue
        if bool(finished[p]):
            out.append((c, p * B * B, p, None, None))
            continue
        srt = [torch.sort(lp[p, s], descending=True, stable=True) for s in range(S)]          # stable: ties in ascending index
        for a in range(K):
            l0, t0 = srt[0].values[a], int(srt[0].indices[a])
            if S == 1:
                out.append((c + l0, (p * B + a) * B, p, (t0,), (l0,)))
            else:
                for b in range(K):
                    l1, t1 = srt[1].values[b], int(srt[1].indices[b])
                    out.append((c + (l0 + l1), (p * B + a) * B + b, p, (t0, t1), (l0, l1)))
    out.sort(key=lambda r: (-float(r[0]), r[1]))
    return out


def select(logits, scores, finished, B, dtype=torch.float64):
    """The selection step on [G * B, S, V] logits: -> dict(parents int32 [G * B] inside the group, tokens int64 [G * B, S], token_lp,
    scores, finished uint8) in `dtype` arithmetic."""
    rows, S, V = logits.shape
    G = rows // B
    lp = _lp(logits, dtype)
    sc = scores.to(dtype)
    res = dict(parents=torch.zeros(rows, dtype=torch.int32), tokens=torch.full((rows, S), -1, dtype=torch.int64),
               token_lp=torch.zeros(rows, S, dtype=dtype), scores=torch.full((rows,), NEG, dtype=dtype),
               finished=torch.ones(rows, dtype=torch.uint8))
    for g in range(G):
        sl = slice(g * B, (g + 1) * B)
        cand = candidates(lp[sl], sc[sl], finished[sl], B)
        for i in range(B):
            r = g * B + i
            res["parents"][r] = i
            if i >= len(cand):
                continue                                   # a dead slot
            score, q, p, toks, lps = cand[i]
            res["parents"][r], res["scores"][r] = p, score
            if toks is not None:
                res["tokens"][r] = torch.tensor(toks)
                res["token_lp"][r] = torch.stack(list(lps))
                res["finished"][r] = 1 if (V - 1) in toks else 0
    return res


def decidable(logits, scores, finished, B) -> bool:
    """fp64: walking the sorted candidates of every group from the best to the first rejected one, neighbours tie exactly or differ by
    more than GAP - no fp32-sized error can change the selection or its order."""
    rows = logits.shape[0]
    lp = _lp(logits, torch.float64)
    for g in range(rows // B):
        sl = slice(g * B, (g + 1) * B)
        cand = candidates(lp[sl], scores[sl].double(), finished[sl], B, extra=1)
        for i in range(min(B, len(cand) - 1)):
            d = float(cand[i][0]) - float(cand[i + 1][0])
            if d != 0.0 and d <= GAP:
                return False
    return True


def _group(kind, B, S, V, gen):
    """logits [B, S, V] on a grid of 1/32 (equal entries tie exactly, others differ by >= 1/32), scores on a grid of 1/8"""
    lg = torch.randint(-320, 321, (B, S, V), generator=gen).to(torch.float32) / 32
    sc = -torch.randint(0, 160, (B,), generator=gen).to(torch.float32) / 8
    fin = torch.zeros(B, dtype=torch.uint8)
    if kind == "mixed":            # identical rows with equal parent scores (exact ties across parents); a finished parent among live ones
        if B >= 2:
            lg[1], sc[1] = lg[0], sc[0]
        if B >= 3:
            fin[2], sc[2] = 1, sc.max() + 1.0
        if B >= 10:
            fin[7], sc[7] = 1, sc[2]                      # two finished hypotheses with the same score
    elif kind == "step0":
        sc[:] = NEG
        sc[0] = 0.0
    else:                          # all finished, two of them with equal scores
        fin[:] = 1
        if B >= 2:
            sc[B - 1] = sc[0]
    return lg, sc, fin


KINDS = ("mixed", "step0", "finished")
BEAMS = (1, 2, 3, 10, 16)
VOCABS = rs.VOCABS             # (1, 3, 5, 502, 1023, 1024): min(B, V) shortlists
_BLOCKS = {}


def block(B, S, V):
    """(logits [3 B, S, V], scores [3 B], finished [3 B]): G = 3 groups - mixed, step 0, all finished; the first seed whose block is
    decidable in fp64."""
    key = (B, S, V)
    if key not in _BLOCKS:
        for seed in range(64):
            gen = torch.Generator().manual_seed(seed * 7919 + B * 131 + S * 17 + V)
            parts = [_group(k, B, S, V, gen) for k in KINDS]
            blk = tuple(torch.cat([p[i] for p in parts]) for i in range(3))
            if decidable(*blk, B):
                _BLOCKS[key] = blk
                break
        else:
            raise AssertionError(f"no decidable block for B = {B}, S = {S}, V = {V}")
    return _BLOCKS[key]


# ---------------------------------------------------------------- records -> sequences
def brute_force_sequences(parents, tokens, logprobs):
    """list-of-lists beam over the records: after every step hypothesis i is its parent's sequence plus the step's entry"""
    T, B = parents.shape
    hyps = [([], []) for _ in range(B)]
    for t in range(T):
        hyps = [(hyps[int(parents[t, i])][0] + [tokens[t, i].tolist()], hyps[int(parents[t, i])][1] + [logprobs[t, i].tolist()]) for i in range(B)]
    return hyps


def replay(parents, tokens, logprobs):
    """The search the records describe, step by step: -> list over steps of lists over slots of (token prefix as a tuple of per-step tuples,
    score) with the score accumulated in fp32 in the selection's association, c[parent] + lp0 or c[parent] + (lp0 + lp1); a carried
    hypothesis (tokens -1) keeps prefix and score; a dead one has score -inf."""
    T, B, S = tokens.shape
    lp32 = logprobs.to(torch.float32)
    cur = [((), torch.tensor(0.0 if i == 0 else NEG, dtype=torch.float32)) for i in range(B)]
    steps = []
    for t in range(T):
        new = []
        for i in range(B):
            pre, c = cur[int(parents[t, i])]
            tk = tuple(tokens[t, i].tolist())
            if tk[0] >= 0:
                pre, c = pre + (tk,), (c + lp32[t, i, 0] if S == 1 else c + (lp32[t, i, 0] + lp32[t, i, 1]))
            elif int(parents[t, i]) == i and not float(c) > NEG:
                c = torch.tensor(NEG, dtype=torch.float32)
            new.append((pre, c))
        cur = new
        steps.append(cur)
    return steps


# ---------------------------------------------------------------- the whole search on the fp64 oracle
def oracle_beam(sd, src, B, max_len):
    """Beam search with fp64 logits from the oracle.  -> list over steps of dict(hyps: list of B (prefix, score, finished, parent),
    margin: the score of the B-th kept candidate minus that of the best rejected one (inf when none was rejected), bound: the
    per-step error bound S * max over the live rows of (2 LONG_LOGIT_TOL ||logits64||_2 + 256 * 2^-24 (1 + |lp64|)) - lp64 over the
    shortlists), ended."""
    import t2s_oracle as orc
    d = orc.t2s_dims(sd)
    S = 2 if d["two_output"] else 1
    V = sd["semantic_token_emb.weight"].shape[0]
    hyps = [((), 0.0 if i == 0 else NEG, False, 0) for i in range(B)]
    out = []
    for t in range(max_len):
        lp = torch.zeros(B, S, V, dtype=torch.float64)
        bound = 0.0
        for p, (pre, c, fin, _) in enumerate(hyps):
            if fin or not c > NEG:
                continue
            st = torch.tensor([list(x) for x in pre] + [[0] * S], dtype=torch.int64).T.reshape(S, -1)      # [S, t + 1]: the last entry is not read
            lg = orc.teacher_forced_logits(sd, src, st, dtype=torch.float64)[-1]                            # [S, V]
            lp[p] = torch.log_softmax(lg, dim=-1)
            top = lp[p].topk(min(B + 1, V), dim=-1).values
            per = 2 * orc.LONG_LOGIT_TOL * lg.norm(dim=-1) + rs.LOGP_TOL_ULPS * rs.EPS * (1.0 + top.abs().max(dim=-1).values)
            bound = max(bound, S * float(per.max()))
        sc = torch.tensor([h[1] for h in hyps], dtype=torch.float64)
        fin = torch.tensor([h[2] for h in hyps])
        cand = candidates(lp, sc, fin, B, extra=1)
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


def decidable_prefix(steps):
    """(number of steps before the first one whose margin is <= twice the accumulated bound, the accumulated bound after every step)"""
    acc, accs, n = 0.0, [], None
    for t, s in enumerate(steps):
        acc += s["bound"]
        accs.append(acc)
        if n is None and s["margin"] <= 2 * acc:
            n = t
    return (len(steps) if n is None else n), accs
