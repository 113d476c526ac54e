"""Shared by tests/test_t2s_beam_rules.py (CPU) and tests/test_t2s_beam_rules_gpu.py: beam search under the history rules no-repeat n-gram
and minimum length (include/covomix_hip.h, cvx_t2s_beam_rules_steps) restated in torch on the CPU, on top of tests/t2s_beam_restated.py
(`candidates`, `select`, the crafted blocks) and tests/t2s_rules_restated.py (`banned_ids`) - the selection step in fp64 and fp32, crafted
histories for the blocks, and the whole search on the fp64 oracle, unguided and guided.  Test infrastructure only.

The points of the definition, as restated here:
  1. h_s of a live hypothesis: the tokens its ancestry took in stream s (given outright to the selection; the prefix in the oracle search);
  2. lp = log_softmax of the row exactly as without rules; the bans are -inf ON lp, afterwards;
  3. n in 1..8: banned_ids(h_s, n);  pos < m: the eos (V - 1), in every stream;
  4. no un-banned entry left in a stream's row: that stream's n-gram bans are void for the step, the eos ban stays;
  5. shortlists rank the banned lp (lp descending, index ascending); a shortlist entry of -inf gives no candidate; a new slot without a
     candidate is dead;
  6. token log-probs and scores are the model's: c[p] + lp0 or c[p] + (lp0 + lp1) over the un-banned lp values."""
import math

import torch

import t2s_beam_restated as br
import t2s_logprob_restated as rs
from t2s_rules_restated import banned_ids

NEG = br.NEG


def ban_row(lp_row, h, n, m):
    """One row: lp_row [V] (any float dtype), h int64 [pos] -> (the banned row, whether the n-gram bans were void)"""
    V = lp_row.numel()
    pos = int(h.numel())
    mark = torch.zeros(V, dtype=torch.bool)
    ids = banned_ids(h, int(n))
    mark[ids[(ids >= 0) & (ids < V)]] = True
    eos = torch.zeros(V, dtype=torch.bool)
    eos[V - 1] = pos < int(m)
    void = bool((mark | eos).all())                     # no un-banned entry: the n-gram bans are void, the eos ban stays
    out = lp_row.clone()
    out[eos if void else (mark | eos)] = NEG
    return out, void


def ban(lp, hists, n, m):
    """One group: lp [B, S, V], hists: B tensors int64 [S, pos_p] -> (banned lp, number of void rows)"""
    out, voids = lp.clone(), 0
    for p in range(lp.shape[0]):
        for s in range(lp.shape[1]):
            out[p, s], v = ban_row(lp[p, s], hists[p][s], n, m)
            voids += int(v)
    return out, voids


def candidates(lp_banned, scores, finished, B, extra=0):
    """t2s_beam_restated.candidates over the banned lp, without the candidates a -inf shortlist entry would give"""
    return [c for c in br.candidates(lp_banned, scores, finished, B, extra) if c[4] is None or all(float(x) > NEG for x in c[4])]


def select(logits, scores, finished, B, history, hist_len, table, dtype=torch.float64):
    """The selection step under the rules on [G * B, S, V] logits; history int [G * B, S, ld], hist_len int [G * B], table int [G, 4]
    ([2] n, [3] m) -> t2s_beam_restated.select's dict plus `voids` (rows whose n-gram bans were void, live hypotheses only)."""
    rows, S, V = logits.shape
    G = rows // B
    lp = br._lp(logits, dtype)
    sc = scores.to(dtype)
    res = dict(parents=torch.zeros(rows, dtype=torch.int32), tokens=torch.full((rows, S), -1, dtype=torch.int64),
               token_lp=torch.zeros(rows, S, dtype=dtype), scores=torch.full((rows,), NEG, dtype=dtype),
               finished=torch.ones(rows, dtype=torch.uint8), voids=0)
    for g in range(G):
        sl = slice(g * B, (g + 1) * B)
        n, m = min(max(int(table[g, 2]), 0), 8), max(int(table[g, 3]), 0)
        hists = [history[g * B + p, :, :min(max(int(hist_len[g * B + p]), 0), history.shape[2])].long() for p in range(B)]
        banned, voids = ban(lp[sl], hists, n, m)
        live = [p for p in range(B) if float(sc[g * B + p]) > NEG and not bool(finished[g * B + p])]
        res["voids"] += sum(int(ban_row(lp[g * B + p, s], hists[p][s], n, m)[1]) for p in live for s in range(S))
        cand = candidates(banned, sc[sl], finished[sl], B)
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


def decidable(logits, scores, finished, B, history, hist_len, table) -> bool:
    """t2s_beam_restated.decidable over the candidates the rules leave: from the best to the first rejected one, neighbours tie exactly
    or differ by more than GAP in fp64"""
    rows = logits.shape[0]
    lp = br._lp(logits, torch.float64)
    for g in range(rows // B):
        sl = slice(g * B, (g + 1) * B)
        n, m = int(table[g, 2]), int(table[g, 3])
        hists = [history[g * B + p, :, :int(hist_len[g * B + p])].long() for p in range(B)]
        cand = candidates(ban(lp[sl], hists, n, m)[0], scores[sl].double(), finished[sl], B, extra=1)
        for i in range(min(B, len(cand) - 1)):
            d = float(cand[i][0]) - float(cand[i + 1][0])
            if d != 0.0 and d <= br.GAP:
                return False
    return True


# ---------------------------------------------------------------- crafted histories for the crafted blocks
def cover_len(V, n) -> int:
    """the shortest history_block(kind="cover") history that bans every id of [0, V - 1)"""
    return n * max(V - 1, 1) + (n - 1)


def history_block(B, S, V, hist_len, n, kind="plain", seed=0):
    """Histories for t2s_beam_restated.block(B, S, V) (3 B rows): int32 [3 B, S, max(hist_len, 1)], ids in [0, max(V - 1, 1)) - a live
    hypothesis has taken no eos.  Every row ENDS in the n - 1 tokens it also holds earlier, followed there by the row's best entries, so
    the n-gram rule bans what the unruled selection would take (when hist_len allows).  kind:
      "plain"  as described;
      "cover"  the ids 0, 1, 2, ... follow that context instead: with hist_len >= cover_len(V, n) EVERY id of [0, V - 1) is banned - with
               the eos banned too (m > hist_len) nothing is left and the bans are void; with the eos free it is each live hypothesis'
               only candidate, so a group with fewer live and finished hypotheses than B gets dead slots."""
    rows = 3 * B
    lg = br.block(B, S, V)[0]
    gen = torch.Generator().manual_seed(seed * 104729 + B * 131 + S * 17 + V + 7 * hist_len + n)
    hi = max(V - 1, 1)
    ld = max(hist_len, 1)
    h = torch.randint(0, hi, (rows, S, ld), generator=gen).to(torch.int32)
    if hist_len < n or n < 1:
        return h
    n1 = n - 1
    ctx = torch.randint(0, hi, (n1,), generator=gen).to(torch.int32)
    for r in range(rows):
        for s in range(S):
            order = torch.sort(lg[r, s, :hi], descending=True, stable=True).indices.to(torch.int32)
            if kind != "plain":
                order = torch.arange(hi, dtype=torch.int32)
            row = h[r, s, :hist_len]
            j, k = 0, 0
            while j + n <= hist_len - n1 and k < order.numel():      # (context, followed-by) groups, up to the closing context
                row[j:j + n1] = ctx
                row[j + n1] = order[k]
                j, k = j + n, k + 1
            if n1:
                row[hist_len - n1:] = ctx
    return h


# ---------------------------------------------------------------- the whole search on the fp64 oracle
def oracle_beam(sd, src, B, max_len, n, m, scale=1.0):
    """t2s_beam_restated.oracle_beam (scale == 1) / t2s_beam_guided_restated.oracle_beam_guided (scale > 1) under the rules: the same
    hypotheses, bounds and margins over the candidates the bans leave, plus per step
      differs: the selection differs from the one the SAME state gives without rules (a banned candidate would have been kept);
      moved:   a hypothesis continues from another slot."""
    import t2s_oracle as orc
    d = orc.t2s_dims(sd)
    S = 2 if d["two_output"] else 1
    V = sd["semantic_token_emb.weight"].shape[0]
    scale = float(scale)
    no_text = torch.zeros(src.numel() + 1)
    hyps = [((), 0.0 if i == 0 else NEG, False, 0) for i in range(B)]
    out = []
    for t in range(max_len):
        lp = torch.zeros(B, S, V, dtype=torch.float64)
        bound = 0.0
        hists = []
        for p, (pre, c, fin, _) in enumerate(hyps):
            hists.append(torch.tensor([list(x) for x in pre], dtype=torch.int64).reshape(-1, S).T.reshape(S, -1))
            if fin or not c > NEG:
                continue
            st = torch.tensor([list(x) for x in pre] + [[0] * S], dtype=torch.int64).T.reshape(S, -1)
            if scale > 1.0:
                lg = orc.teacher_forced_logits(sd, src, st, cond_scale=scale, dtype=torch.float64)[-1]
                cond = orc.teacher_forced_logits(sd, src, st, dtype=torch.float64)[-1]
                null = orc.teacher_forced_logits(sd, src, st, dtype=torch.float64, context_mask=no_text)[-1]
                norm = scale * cond.norm(dim=-1) + (scale - 1.0) * null.norm(dim=-1)
            else:
                lg = orc.teacher_forced_logits(sd, src, st, dtype=torch.float64)[-1]
                norm = lg.norm(dim=-1)
            lp[p] = torch.log_softmax(lg, dim=-1)
            top = lp[p].topk(min(B + 1, V), dim=-1).values
            per = 2 * orc.LONG_LOGIT_TOL * norm + rs.LOGP_TOL_ULPS * rs.EPS * (1.0 + top.abs().max(dim=-1).values)
            bound = max(bound, S * float(per.max()))
        sc = torch.tensor([h[1] for h in hyps], dtype=torch.float64)
        fin = torch.tensor([h[2] for h in hyps])
        live = [p for p, h in enumerate(hyps) if not h[2] and h[1] > NEG]
        banned = lp.clone()
        for p in live:
            for s in range(S):
                banned[p, s] = ban_row(lp[p, s], hists[p][s], n, m)[0]
        cand = candidates(banned, sc, fin, B, extra=1)
        plain = br.candidates(lp, sc, fin, B)
        margin = float(cand[B - 1][0]) - float(cand[B][0]) if len(cand) > B else math.inf
        differs = {c[1:4] for c in cand[:B]} != {c[1:4] for c in plain[:B]}
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
        out.append(dict(hyps=hyps, margin=margin, bound=bound, ended=ended, differs=differs,
                        moved=any(h[3] != i and h[1] > NEG for i, h in enumerate(hyps))))
        if ended:
            break
    return out


# the oracle cases of the CPU and the GPU test: (fixture, ids of its golden text, beam size, n, m, guidance scale)
MAX_LEN = 40
ORACLE_CASES = [("cosingle_small", 12, 3, 2, 9, 1.0), ("cosingle_small", 12, 3, 3, 9, 1.0), ("comix_small", 12, 2, 3, 9, 1.0),
                ("cosingle_small", 12, 3, 2, 9, 1.5)]
_CACHE: dict = {}


def oracle_case(sd, src_full, case):
    """(steps, decidable prefix, accumulated bounds, steps of the prefix whose selection the rules changed, re-parenting steps of the
    prefix) of one case, computed once per process"""
    if case not in _CACHE:
        name, ids, B, n, m, scale = case
        steps = oracle_beam(sd, src_full[:, :ids], B, MAX_LEN, n, m, scale)
        k, acc = br.decidable_prefix(steps)
        _CACHE[case] = (steps, k, acc, sum(1 for s in steps[:k] if s["differs"]), sum(1 for s in steps[:k] if s["moved"]))
    return _CACHE[case]


# ---------------------------------------------------------------- properties of a returned hypothesis
def repeats(streams, n: int) -> int:
    """n-grams that occur a second time in any stream of streams [S, L]"""
    from t2s_rules_restated import repeated_ngrams
    return sum(repeated_ngrams(row.tolist(), n) for row in streams)
