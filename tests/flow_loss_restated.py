"""The flow-matching loss restated on the host (numpy / torch, no GPU): what tests/test_flow_loss.py and tests/test_flow_loss_gpu.py
compare the kernels, VectorField.evaluate_seq_times and CoVoMixModel.flow_matching_loss with.

  cfm_inputs       the inputs kernel in individually rounded fp32 numpy operations, in the kernel's stated order (compared with ==)
  cfm_inputs64     the same formulas in fp64
  masked_loss64    acoustic.py:527-536 for one utterance in fp64
  utterance        seeded synthetic inputs of one utterance (tokens, mel, conditioning mel, noise, mask)
  oracle_utterance pred, flow and the loss of one utterance in fp64 on covomix_oracle.acoustic_forward (one time per batch item)

Written from the reference's formulas (acoustic.py:773, :775, :469, :527-536), not from covomix_amd."""
import numpy as np
import torch

F32 = np.float32


def cfm_inputs(x1, x0, cond, mask, times_rows, sigma):
    """numpy fp32: x1, x0 [M, D], cond [M, C], mask bool [M], times_rows fp32 [M] (the time of every row's sequence) -> (w, flow, cond_in).
    Every operation is one rounded fp32 operation: a = 1 - sigma; b = a t; c = 1 - b; w = c x0 + t x1; flow = x1 - a x0."""
    x1, x0, cond = (np.ascontiguousarray(v, dtype=F32) for v in (x1, x0, cond))
    t = np.asarray(times_rows, dtype=F32)[:, None]
    a = F32(1.0) - F32(sigma)
    b = (a * t).astype(F32)
    c = (F32(1.0) - b).astype(F32)
    p, q = (c * x0).astype(F32), (t * x1).astype(F32)
    w = (p + q).astype(F32)
    flow = (x1 - (a * x0).astype(F32)).astype(F32)
    cond_in = np.where(np.asarray(mask, dtype=bool)[:, None], F32(0.0), cond).astype(F32)
    return w, flow, cond_in


def cfm_inputs64(x1, x0, cond, mask, times_rows, sigma):
    x1, x0, cond = (np.asarray(v, dtype=np.float64) for v in (x1, x0, cond))
    t = np.asarray(times_rows, dtype=np.float64)[:, None]
    s = float(F32(sigma))
    return (1 - (1 - s) * t) * x0 + t * x1, x1 - (1 - s) * x0, cond * (~np.asarray(mask, dtype=bool))[:, None]


def masked_loss64(pred, flow, mask):
    """(loss, err_rows) of one utterance in fp64: err_rows = mean_d (pred - flow)^2; loss = sum over masked rows / max(count, 1e-5)."""
    e = (pred.double() - flow.double()).square().mean(dim=-1)
    m = mask.bool()
    return float(e.masked_fill(~m, 0.0).sum() / max(float(m.sum()), 1e-5)), e


def utterance(kind: str, T: int, seed: int) -> dict:
    """One synthetic utterance: phoneme_ids [T(, 2)], mel [T, 80] ~ N(-6, 2^2) clipped as synthetic.synthetic_inputs draws it, cond [T, C]
    (VoSingle: the mel itself, VoMix: a 160-wide mel of its own), x0 [T, 80] ~ N(0, 1), mask bool [T] (a span of ~60 % from T // 5, never
    empty, never full for T >= 2)."""
    g = torch.Generator().manual_seed(seed)
    two = kind == "vomix"
    ids = torch.randint(0, 501, (T, 2) if two else (T,), generator=g)
    mel = (torch.randn(T, 80, generator=g) * 2.0 - 6.0).clamp(-11.52, 2.0)
    cond = (torch.randn(T, 160, generator=g) * 2.0 - 6.0).clamp(-11.52, 2.0) if two else mel.clone()
    x0 = torch.randn(T, 80, generator=g)
    mask = torch.zeros(T, dtype=torch.bool)
    lo = T // 5
    mask[lo:lo + max(1, (3 * T) // 5)] = True
    return dict(phoneme_ids=ids, mel=mel, cond=cond, x0=x0, mask=mask)


def oracle_utterance(sd64: dict, u: dict, t: float, sigma: float = 0.0, drop: bool = False) -> dict:
    """fp64: pred, flow, err_rows and the loss of one utterance at time t (fp32-representable), B = 1 on the oracle."""
    import covomix_oracle as orc
    T = u["mel"].shape[0]
    t32 = float(F32(t))
    w, flow, cond_in = cfm_inputs64(u["mel"].numpy(), u["x0"].numpy(), u["cond"].numpy(), u["mask"].numpy(), np.full(T, t32), sigma)
    w, flow, cond_in = (torch.from_numpy(np.ascontiguousarray(v)) for v in (w, flow, cond_in))
    pred = orc.acoustic_forward(sd64, w[None], torch.tensor([t32], dtype=torch.float64), u["phoneme_ids"][None], cond_in[None], drop)[0]
    loss, err = masked_loss64(pred, flow, u["mask"])
    return dict(pred=pred, flow=flow, err_rows=err, loss=loss)
