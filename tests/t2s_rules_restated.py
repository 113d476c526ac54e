"""Plain-torch restatement (fp32, as the device computes them) of the HISTORY RULES of the text2semantic decode - repetition penalty,
no-repeat n-gram, minimum length, and the void-ban fallback (the definition: include/covomix_hip.h, cvx_t2s_decode_steps_rules) - and of the
decode they lead to on given logits.  The checker of tests/test_t2s_rules.py (pinned there against a brute-force loop) and of
tests/test_t2s_rules_gpu.py.  Test infrastructure only.

A rule set is the tuple (theta, W, n, m) of covomix_amd.t2s.check_rules.  h: the tokens one output stream has emitted, pos = len(h).
  1. every id in h[max(0, pos - W):pos] (W = 0: all of h) is penalised once: l = l / theta where l > 0, l * theta elsewhere (fp32, IEEE);
  2. n >= 1: for every j in [0, pos - n] with h[j:j + n - 1] == h[pos - n + 1:pos] the id h[j + n - 1] becomes -inf;
  3. pos < m: the eos becomes -inf.
No finite entry after 3: the bans of 2 are void for this step, 1 and 3 stay."""
import torch

import t2s_filter_restated as fr

OFF = (1.0, 0, 0, 0)


def penalised_ids(h: torch.Tensor, W: int) -> torch.Tensor:
    pos = h.numel()
    return torch.unique(h[max(0, pos - W) if W > 0 else 0:])


def banned_ids(h: torch.Tensor, n: int) -> torch.Tensor:
    """the ids that would complete an n-gram h already holds (n = 1: every id of h); none while h holds fewer than n tokens"""
    pos = h.numel()
    if n < 1 or pos < n:
        return h[:0]
    windows = h.unfold(0, n, 1)                                       # [pos - n + 1, n]: window j = h[j:j + n]
    match = (windows[:, :n - 1] == h[pos - n + 1:][None, :]).all(dim=1)
    return torch.unique(windows[match, n - 1])


def apply_rules(logits: torch.Tensor, h: torch.Tensor, rules, eos: int):
    """One row: logits fp32 [V], h int64 [pos] -> (the row the filter sees, fp32 [V]; whether the bans were void)"""
    theta, W, n, m = rules
    l = logits.detach().cpu().to(torch.float32).clone()
    h = torch.as_tensor(h, dtype=torch.int64).reshape(-1)
    th = torch.tensor(float(theta), dtype=torch.float32)
    pen = torch.zeros(l.numel(), dtype=torch.bool)
    pen[penalised_ids(h, int(W))] = True
    l = torch.where(pen, torch.where(l > 0, l / th, l * th), l)
    if h.numel() < int(m):
        l[eos] = float("-inf")
    out = l.clone()
    out[banned_ids(h, int(n))] = float("-inf")
    if not bool(torch.isfinite(out).any()):
        return l, True
    return out, False


def delta_for(rules, delta: float = fr.DELTA) -> float:
    """The decidability margin under a rule set: the penalty maps a logit through a continuous, piecewise linear function of slope
    1 / theta or theta, so a change of a logit by less than delta / 2 moves the ruled logit by less than max(theta, 1 / theta) delta / 2;
    bans and the eos suppression depend on the history alone."""
    theta = float(rules[0])
    return delta * max(theta, 1.0 / theta)


def restated_decode_choice(logits_per_step: torch.Tensor, uniforms: torch.Tensor, settings, rules, tokens=None, eos=None):
    """The decode on GIVEN logits: logits_per_step fp32 [L, S, V] (the model's rows, before the rules), uniforms [>= L, S, V], settings =
    (temperature, mode, k, thres) (t2s_filter_restated), rules = (theta, W, n, m).  Per step and stream: the rules on the row with the
    stream's history, then the filter, then the choice (t2s_filter_restated.restated_choice).  The history is built from the function's
    own choices - or, with `tokens` int64 [L, S], from those (the tokens a decode under test emitted: one flipped undecidable step then
    does not derail the steps behind it).  eos: default V - 1.
    -> (tokens int64 [L, S], decidable bool [L, S] as in t2s_filter_restated at the margin delta_for(rules), the number of fallback steps)"""
    temperature, mode, k, thres = settings
    lg = logits_per_step.detach().cpu().to(torch.float32)
    L, S, V = lg.shape
    eos = V - 1 if eos is None else int(eos)
    out = torch.zeros(L, S, dtype=torch.int64)
    ok = torch.zeros(L, S, dtype=torch.bool)
    fallbacks = 0
    delta = delta_for(rules)
    hist = out if tokens is None else torch.as_tensor(tokens).detach().cpu().to(torch.int64)
    for t in range(L):
        for s in range(S):
            row, void = apply_rules(lg[t, s], hist[:t, s], rules, eos)
            fallbacks += int(void)
            tk, dec = fr.restated_choice(row[None], uniforms[t, s][None], temperature, mode, k, thres, delta)
            out[t, s], ok[t, s] = tk[0], dec[0]
    return out, ok, fallbacks


def repeated_ngrams(h, n: int) -> int:
    """how many n-grams of the sequence h occur a second (third, ...) time"""
    h = [int(x) for x in h]
    seen, rep = set(), 0
    for j in range(len(h) - n + 1):
        g = tuple(h[j:j + n])
        rep += g in seen
        seen.add(g)
    return rep
