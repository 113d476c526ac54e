"""Plain-torch restatement (fp64) of the reference's logit filters `top_k` / `top_p` (covomix/covomix_model/text2semantic.py:118-132)
and of the token they lead to - the checker of tests/test_t2s_filters.py (pinned there against the reference's own masks,
tests/golden/t2s_filters.npz) and of tests/test_t2s_filters_gpu.py.  Test infrastructure only.

  top-k  entry i is kept iff fewer than k logits are LARGER than it: the k largest, and with them every entry that equals the k-th
         (torch.topk picks k and leaves open which of the equal ones; the decode has always kept them all, by rank counting);
  top-p  entry i is kept iff the softmax mass of the entries sorted before it is <= thres (F.pad(cum_probs > thres, (1, -1))), where
         entry j is "sorted before" entry i when l_j > l_i, or l_j == l_i and j < i (the stable descending order; torch.sort
         leaves the order of ties open)."""
import math

import torch

TOP_K, TOP_P = 0, 1
DELTA = 1e-3                     # == oracle/t2s_oracle.DELTA (reference_choice)


def sorted_before(l: torch.Tensor) -> torch.Tensor:
    """l [..., V] -> bool [..., V, V]: [.., i, j] = entry j is sorted before entry i"""
    V = l.shape[-1]
    idx = torch.arange(V)
    li, lj = l[..., :, None], l[..., None, :]
    return (lj > li) | ((lj == li) & (idx[None, :] < idx[:, None]))


def kept_mask(logits: torch.Tensor, mode: int, k: int = 0, thres: float = 0.0) -> torch.Tensor:
    l = logits.double().cpu()
    if mode == TOP_K:
        return (l[..., None, :] > l[..., :, None]).sum(dim=-1) < k
    before = sorted_before(l)
    p = torch.softmax(l, dim=-1)
    return (before.double() @ p[..., :, None])[..., 0] <= thres


def filtered(logits: torch.Tensor, mode: int, k: int = 0, thres: float = 0.0) -> torch.Tensor:
    """the reference's filter output: the logits where kept, -inf elsewhere (dtype of the input)"""
    return logits.masked_fill(~kept_mask(logits, mode, k, thres).to(logits.device), float("-inf"))


def gumbel(u: torch.Tensor) -> torch.Tensor:
    log = lambda t: torch.log(t.clamp(min=1e-20))
    return -log(-log(u))


def score_of(logits, uniforms, kept, temperature: float) -> torch.Tensor:
    l, u = logits.double().cpu(), uniforms.double().cpu()
    return (l / max(temperature, 1e-10) + gumbel(u)).masked_fill(~kept, float("-inf"))


def margin_ok(score: torch.Tensor, delta: float = DELTA) -> torch.Tensor:
    """top-2 margin of the score above delta (a row with one kept entry: margin inf)"""
    top2 = score.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]) > delta


def restated_choice(logits: torch.Tensor, uniforms: torch.Tensor, temperature: float, mode: int, k: int = 0, thres: float = 0.0,
                    delta: float = DELTA):
    """The reference's token for every row of `logits` [..., V] with the draws `uniforms` [..., V]: filter, then argmax of
    filtered / temperature + gumbel (text2semantic.py:105-132, :796-800), in fp64.  Returns (tokens [...], decidable [...] bool), in the
    spirit of oracle/t2s_oracle.reference_choice: a row is decidable when a change of every logit by less than delta / 2 cannot
    change the token -
      * the winner's score beats the runner-up of the kept set by more than delta;
      * the winner is not NEAR the filter's boundary, and no entry near the boundary scores within delta of the winner.
    Near the boundary: top-k - within delta of the midpoint between the k-th and the (k+1)-th logit (none when k == V).
    top-p - an entry is surely kept when the mass of every entry that a change could sort before it (l_j >= l_i - delta, j != i)
    plus 2 delta (a sum of softmax masses is <= 1 and moves by less than delta either way) is still <= thres, surely
    dropped when the mass of the entries that stay before it (l_j > l_i + delta) minus 2 delta is still > thres, near otherwise."""
    l = logits.double().cpu()
    kept = kept_mask(l, mode, k, thres)
    score = score_of(l, uniforms, kept, temperature)
    tokens = score.argmax(dim=-1)
    best = score.max(dim=-1).values
    if mode == TOP_K:
        V = l.shape[-1]
        if k < V:
            srt = l.sort(dim=-1, descending=True).values
            boundary = 0.5 * (srt[..., k - 1] + srt[..., k])
            near = (l - boundary[..., None]).abs() < delta
        else:
            near = torch.zeros_like(kept)
    else:
        p = torch.softmax(l, dim=-1)
        li, lj = l[..., :, None], l[..., None, :]
        eye = torch.eye(l.shape[-1], dtype=torch.bool)
        maybe = ((lj >= li - delta) & ~eye).double() @ p[..., :, None]
        surely = (lj > li + delta).double() @ p[..., :, None]
        sure_kept = maybe[..., 0] + 2 * delta <= thres
        sure_dropped = surely[..., 0] - 2 * delta > thres
        near = ~(sure_kept | sure_dropped)
    raw = l / max(temperature, 1e-10) + gumbel(uniforms.double().cpu())
    winner_near = near.gather(-1, tokens[..., None])[..., 0]
    rival = (near & (raw > best[..., None] - delta)).scatter(-1, tokens[..., None], False).any(dim=-1)
    return tokens, margin_ok(score, delta) & ~winner_near & ~rival


def setting(name: str, vocab: int, **kw):
    """(mode, k, thres) as covomix_amd.t2s.filter_setting resolves the reference's arguments"""
    if name == "top_k":
        k = kw.get("k")
        return (TOP_K, math.ceil(kw.get("thres", 0.1) * vocab) if k is None else int(k), 0.0)
    return (TOP_P, 0, float(kw.get("thres", 0.9)))
