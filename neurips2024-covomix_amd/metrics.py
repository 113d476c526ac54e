"""How far a generated mel is from a target mel: the frame-wise MSE the reference validates the acoustic model with
(covomix/util/inference.py:32-75, :151-227: F.mse_loss over the generated part) and, for outputs whose timing is their own (anything
sampled from text2semantic tokens), the mel-cepstral distortion along a dynamic-time-warping path (MCD-DTW; the CoVoMix paper reports
it for the acoustic models).

THIS PROJECT'S DEFINITION of the cepstrum: coefficients 1 ... n_coef of the orthonormal DCT-II of the 80-bin natural-log mel that
mel.py and the sampler produce.  The paper's extraction tool is not part of the reference, so figures are comparable only within this
definition, not with published ones.  Nor does a figure from the small or synthetic models of this repository (random weights) say
anything about audio quality.

The cepstra of all utterances come from ONE call of the exact-fp32 GEMM (ops.gemm), the alignment of all pairs from ONE launch of the
DTW kernel (ops.dtw, csrc/dtw.hip); the division by the path length and the dB constant are finished in fp64 on the host."""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, ops

MCD_DB = 10.0 / math.log(10.0) * math.sqrt(2.0)        # (10 / ln 10) sqrt(2): a Euclidean cepstral distance -> dB


def dct_matrix(n_mels: int = 80, n_coef: int = 13) -> torch.Tensor:
    """fp32 [n_coef, n_mels], built in fp64: rows k = 1 ... n_coef of the orthonormal DCT-II, sqrt(2 / n_mels) cos(pi k (2 m + 1) /
    (2 n_mels)).  c_0, the energy term, is dropped; n_coef <= n_mels - 1."""
    n_mels, n_coef = int(n_mels), int(n_coef)
    if not 1 <= n_coef <= n_mels - 1:
        raise ValueError(f"dct_matrix: n_coef = {n_coef} for {n_mels} mel bins (1 ... n_mels - 1)")
    k = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return torch.from_numpy((math.sqrt(2.0 / n_mels) * np.cos(math.pi * k * (2 * m + 1) / (2 * n_mels))).astype(np.float32))


def _mel_list(mels, what: str) -> list:
    mels = list(mels)
    for i, m in enumerate(mels):
        if not isinstance(m, torch.Tensor) or m.dtype != torch.float32 or m.dim() != 2:
            raise TypeError(f"{what}: mel {i} must be a 2-D float32 tensor [frames, n_mels]")
    if len(set(m.shape[1] for m in mels)) > 1:
        raise ValueError(f"{what}: mels of different widths {sorted(set(m.shape[1] for m in mels))} in one call")
    return mels


def _device_of(tensors):
    on_dev = [t for t in tensors if t.is_cuda]
    if on_dev:
        return on_dev[0].device
    if not torch.cuda.is_available():
        raise _lib.CovomixHipError("the mel metrics need a GPU: covomix_amd has no CPU path")
    return torch.device("cuda")


def mel_cepstrum(mels: Sequence[torch.Tensor], n_coef: int = 13) -> list:
    """mels: a list of [T_i, 80] natural-log mels (host or device) -> a list of [T_i, n_coef] cepstra on the device (this project's
    definition, see the module).  All rows go through ONE ops.gemm call on the exact-fp32 GEMM, which adds the products of an element
    in one order in every form: an utterance's cepstra do not depend on its neighbours in the call."""
    mels = _mel_list(mels, "mel_cepstrum")
    if not mels:
        return []
    w_host = dct_matrix(mels[0].shape[1], n_coef)
    dev = _device_of(mels)
    rows = torch.cat([m.to(dev) for m in mels]).contiguous()
    out = torch.empty(rows.shape[0], w_host.shape[0], dtype=torch.float32, device=dev)
    if rows.shape[0]:
        with torch.cuda.device(dev):
            ops.gemm(rows, ops.h2d(w_host, dev), out)
    return list(out.split([m.shape[0] for m in mels]))


def mel_cepstral_distortion(pred: Sequence[torch.Tensor], ref: Sequence[torch.Tensor], n_coef: int = 13, align: str = "dtw") -> tuple:
    """Mel-cepstral distortion of pred[i] against ref[i] -> (mcd float64 [P] in dB, steps int32 [P]), on the host:
        mcd = (10 / ln 10) sqrt(2) * cost / steps
    with cost the sum of the Euclidean distances between the cepstra (mel_cepstrum) of the aligned frames and steps their number.
    align="dtw": the best warping path of ops.dtw (all pairs in one launch); lengths may differ.  align="none": frame i against frame
    i, which requires equal lengths (the distances are summed with torch on the device: glue, off the hot path).  A side without
    frames gives NaN.
    THIS PROJECT'S DEFINITION: cepstra 1 ... n_coef of the orthonormal DCT-II of the 80-bin natural-log mel.  The paper's extraction
    tool is not in the reference, so figures are comparable only within this definition; figures from random-weight models say
    nothing about audio quality."""
    pred, ref = _mel_list(pred, "mel_cepstral_distortion"), _mel_list(ref, "mel_cepstral_distortion")
    if len(pred) != len(ref):
        raise ValueError(f"mel_cepstral_distortion: {len(pred)} predictions for {len(ref)} references")
    if align not in ("dtw", "none"):
        raise ValueError(f"mel_cepstral_distortion: align = {align!r} ('dtw' or 'none')")
    P = len(pred)
    if P == 0:
        return torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.int32)
    if align == "none":
        for i, (a, b) in enumerate(zip(pred, ref)):
            if a.shape[0] != b.shape[0]:
                raise ValueError(f"mel_cepstral_distortion: align='none' and pair {i} has {a.shape[0]} and {b.shape[0]} frames")
    cep = mel_cepstrum(pred + ref, n_coef)
    if align == "dtw":
        cost, steps = ops.dtw(cep, [(i, P + i) for i in range(P)])
        cost = cost.double()
    else:
        cost = torch.stack([(a - b).square().sum(dim=1).sqrt().double().sum() for a, b in zip(cep[:P], cep[P:])]).cpu()
        steps = torch.tensor([a.shape[0] for a in pred], dtype=torch.int32)
    mcd = torch.where(steps > 0, MCD_DB * cost / steps.clamp_min(1).double(), torch.full_like(cost, math.nan))
    return mcd, steps


def mel_mse(pred, ref):
    """F.mse_loss(pred, ref), the reference's own measure (covomix/util/inference.py:71, :223): one pair -> a 0-D tensor, lists -> a
    list of them.  Both sides have the same shape."""
    if isinstance(pred, (list, tuple)) != isinstance(ref, (list, tuple)):
        raise ValueError("mel_mse: one pair of mels, or two lists")
    if not isinstance(pred, (list, tuple)):
        if pred.shape != ref.shape:
            raise ValueError(f"mel_mse: shapes {tuple(pred.shape)} and {tuple(ref.shape)}")
        return F.mse_loss(pred, ref.to(pred.device))
    if len(pred) != len(ref):
        raise ValueError(f"mel_mse: {len(pred)} predictions for {len(ref)} references")
    return [mel_mse(a, b) for a, b in zip(pred, ref)]
