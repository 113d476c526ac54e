"""Host side of the acoustic model's flow-matching validation loss (CoVoMixModel.flow_matching_loss): the record it returns, the
random draws of what the caller does not pass, the checks, and the cut of the caller's order into packed launches.

Reference: `valid_loss` of covomix/conditional_model.py:229-271 = ConditionalFlowMatcherWrapper.forward (acoustic.py:732-791) on
CoVoMix.forward(..., target = flow) (:430-538).  The draws follow the reference's DISTRIBUTIONS (times ~ U[0, 1), x0 ~ N(0, 1), the
mask of :460-465), from a CPU torch.Generator in the order documented at `draw` - not the reference's device RNG stream.
No tensor here touches a GPU."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

FRAC_LENGTHS_MASK = (0.7, 1.0)      # CoVoMix.frac_lengths_mask (acoustic.py:344)
P_DROP = 0.3                        # CoVoMix.p_drop_prob (:343)


@dataclass
class FlowLoss:
    """loss: the mean over utterances of per_utterance (fp64, on the host); per_utterance float64 [n]: the masked mean over an utterance's
    frames of the mean over channels of (pred - flow)^2 (the reference at B = 1, acoustic.py:527-538); frames int64 [n]: the masked frames
    that mean is over (0: the loss is 0 through the clamp); times float32 [n]; masks: list of bool [T_i]; err_rows: list of float32 [T_i],
    mean_d (pred - flow)^2 of EVERY frame (masked or not); pred (return_pred): list of float32 [T_i, dim_out], the network's output."""
    loss: float
    per_utterance: torch.Tensor
    frames: torch.Tensor
    times: torch.Tensor
    masks: List[torch.Tensor]
    err_rows: List[torch.Tensor]
    pred: Optional[List[torch.Tensor]] = None


def span_mask(T: int, frac: float, u: float) -> torch.Tensor:
    """mask_from_frac_lengths (acoustic.py:81-94) for one sequence: length = int(frac * T) frames (the product in fp32, truncated)
    starting at int((T - length) * u) (fp32, truncated): the span lies inside the sequence for 0 <= frac <= 1, 0 <= u < 1."""
    length = int((torch.tensor(frac, dtype=torch.float32) * T).long())
    length = max(0, min(T, length))
    start = int((torch.tensor(float(T - length), dtype=torch.float32) * torch.tensor(u, dtype=torch.float32)).clamp(min=0).long())
    start = min(start, T - length)
    m = torch.zeros(T, dtype=torch.bool)
    m[start:start + length] = True
    return m


def draw_mask(T: int, gen: torch.Generator) -> torch.Tensor:
    """The training mask of acoustic.py:460-465 for one sequence.  Draws, in this order: the coin (one U[0, 1): below 0.5 the span);
    for the span f = 0.7 + 0.3 U and the start's U; otherwise T uniforms, a frame is masked where its uniform is below 0.3."""
    if float(torch.rand(1, generator=gen)) < 0.5:
        lo, hi = FRAC_LENGTHS_MASK
        f = lo + (hi - lo) * float(torch.rand(1, generator=gen))
        return span_mask(T, f, float(torch.rand(1, generator=gen)))
    return torch.rand(T, generator=gen) < P_DROP


def draw(lengths: Sequence[int], dim_out: int, seed: Optional[int], need_times: bool = True, need_x0: bool = True,
         need_masks: bool = True) -> dict:
    """What a call does not pass, from ONE CPU torch.Generator seeded with `seed` (None: a fresh random seed).  Utterance by utterance in
    the caller's order, and for each: its time (one U[0, 1) fp32), its noise (randn [T_i, dim_out] fp32), its mask (draw_mask) - a kind
    the caller passed is skipped for every utterance, so the draws of the others keep this order among themselves."""
    gen = torch.Generator()
    if seed is None:
        gen.seed()
    else:
        gen.manual_seed(int(seed))
    out = dict(times=[], x0=[], masks=[])
    for T in lengths:
        if need_times:
            out["times"].append(float(torch.rand(1, generator=gen)))
        if need_x0:
            out["x0"].append(torch.randn(int(T), dim_out, generator=gen))
        if need_masks:
            out["masks"].append(draw_mask(int(T), gen))
    return out


def cut_launches(lengths: Sequence[int], max_rows: int, max_seqs: int) -> List[range]:
    """The caller's order cut into consecutive launches of at most max_rows packed rows and max_seqs utterances (an utterance longer than
    max_rows runs alone)."""
    if isinstance(max_rows, bool) or not isinstance(max_rows, int) or max_rows < 1:
        raise ValueError(f"max_rows = {max_rows!r}: a positive integer")
    out, start, rows = [], 0, 0
    for i, T in enumerate(lengths):
        if i > start and (rows + T > max_rows or i - start >= max_seqs):
            out.append(range(start, i))
            start, rows = i, 0
        rows += T
    out.append(range(start, len(lengths)))
    return out


def check_inputs(d: dict, phoneme_ids, mels, cond_mels, masks, times, x0, cond_drop, sigma) -> dict:
    """Every refusal of flow_matching_loss that needs no device (ValueError / TypeError), and the inputs as CPU tensors:
    d = the model's dimensions (acoustic._dims_from_state)."""
    what = "flow_matching_loss"
    lists = dict(phoneme_ids=phoneme_ids, mels=mels, cond_mels=cond_mels, masks=masks, x0=x0)
    for k, v in lists.items():
        if v is not None and not isinstance(v, (list, tuple)):
            raise ValueError(f"{what}: {k} must be a list of per-utterance tensors")
    n = len(phoneme_ids)
    if n == 0:
        raise ValueError(f"{what}: no utterance")
    for k, v in lists.items():
        if v is not None and len(v) != n:
            raise ValueError(f"{what}: {len(v)} {k} for {n} utterances")
    for k, v in (("times", times), ("cond_drop", cond_drop)):
        if v is not None and len(v) != n:
            raise ValueError(f"{what}: {len(v)} {k} for {n} utterances")
    if not (isinstance(sigma, (int, float)) and 0.0 <= float(sigma) <= 1.0):
        raise ValueError(f"{what}: sigma = {sigma!r} outside [0, 1]")
    conds = mels if cond_mels is None else cond_mels
    lengths = []
    for i in range(n):
        T = int(mels[i].shape[0])
        if mels[i].dim() != 2 or mels[i].shape[1] != d["dim_out"] or T < 1:
            raise ValueError(f"{what}: mels[{i}] must be [T >= 1, {d['dim_out']}], got {tuple(mels[i].shape)}")
        expect = (T,) + ((d["streams"],) if d["streams"] > 1 else ())
        if tuple(phoneme_ids[i].shape) != expect:
            raise ValueError(f"{what}: utterance {i} has {T} mel frames and tokens of shape {tuple(phoneme_ids[i].shape)} ({expect} is needed)")
        if tuple(conds[i].shape) != (T, d["dim_cond"]):
            raise ValueError(f"{what}: the conditioning mel of utterance {i} must be {(T, d['dim_cond'])}, got {tuple(conds[i].shape)}"
                             + ("" if cond_mels is not None else " (cond_mels defaults to mels only where the widths agree)"))
        if masks is not None and (tuple(masks[i].shape) != (T,) or masks[i].dtype != torch.bool):
            raise ValueError(f"{what}: masks[{i}] must be bool [{T}], got {masks[i].dtype} {tuple(masks[i].shape)}")
        if x0 is not None and tuple(x0[i].shape) != (T, d["dim_out"]):
            raise ValueError(f"{what}: x0[{i}] must be {(T, d['dim_out'])}, got {tuple(x0[i].shape)}")
        lengths.append(T)
    tv = None
    if times is not None:
        tv = torch.tensor([float(t) for t in times], dtype=torch.float64).to(torch.float32)
        for i, t in enumerate(tv.tolist()):
            if not 0.0 <= t <= 1.0:          # (NaN fails both comparisons)
                raise ValueError(f"{what}: times[{i}] = {t!r} outside [0, 1]")
    drop = [False] * n if cond_drop is None else [bool(x) for x in cond_drop]
    return dict(n=n, lengths=lengths, conds=conds, times=tv, drop=drop)
