#!/usr/bin/env python3
"""Generate tests/golden/t2s_filters.npz: rows of logits and the kept masks the REFERENCE's own logit filters give them
(`top_k` and `top_p` of covomix/covomix_model/text2semantic.py:118-132, imported from /root/reference, which exists only in the
build container).

Run from the repo root:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_t2s_filters.py

Nothing of the reference travels: only the logits, the settings and the masks (`filtered > -inf`) are saved.  `beartype` (absent
here) is replaced by the no-op shim of make_golden_t2s.py.

Two blocks: V = 503 (not a multiple of 4: the kernels read whole 4-vectors over a padded tail) and V = 1024 (the kernels' limit).
Rows: randn * 3, rows with one dominant entry, nearly flat rows.  A row is kept only when every setting is DECIDED with room, so
that a test excludes nothing and tolerates nothing:
  * top-p: no cumulative softmax mass (fp64, descending order) within 1e-4 of a threshold;
  * top-k: the k-th and the (k+1)-th largest logit are more than 1e-6 apart
and the reference's fp32 masks must equal the fp64 restatement of both rules (asserted below).
"""
import math
import os
import sys
import types
import typing

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "t2s_filters.npz")
sys.dont_write_bytecode = True

ROWS = {503: 28, 1024: 24}                       # rows per block (the file stays under 300 KB)
P_MARGIN, K_MARGIN = 1e-4, 1e-6


def _install_shims():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    bt = mod("beartype", beartype=lambda f: f)
    bt.typing = mod("beartype.typing", Tuple=typing.Tuple, Optional=typing.Optional, List=typing.List,
                    Union=typing.Union, Callable=typing.Callable, Literal=typing.Literal)
    bt.door = mod("beartype.door", is_bearable=lambda obj, t: isinstance(obj, torch.Tensor) and obj.is_floating_point())


def settings(V: int):
    """(name, mode, k, thres): mode 0 top-k (k resolved as the reference resolves it), 1 top-p"""
    return [("top_k k=1", 0, 1, 0.0), ("top_k k=51", 0, 51, 0.0), (f"top_k k={V}", 0, V, 0.0),
            ("top_k thres=0.25", 0, math.ceil(0.25 * V), 0.25),
            ("top_p thres=0.5", 1, 0, 0.5), ("top_p thres=0.9", 1, 0, 0.9), ("top_p thres=0.99", 1, 0, 0.99)]


def decided(row: torch.Tensor, sets) -> bool:
    l = row.double()
    srt = l.sort(descending=True).values
    cum = torch.softmax(srt, dim=-1).cumsum(dim=-1)
    for _, mode, k, thres in sets:
        if mode == 1 and float((cum - thres).abs().min()) <= P_MARGIN:
            return False
        if mode == 0 and k < l.numel() and float(srt[k - 1] - srt[k]) <= K_MARGIN:
            return False
    return True


def fp64_mask(row: torch.Tensor, mode: int, k: int, thres: float) -> torch.Tensor:
    l = row.double()
    V = l.numel()
    bigger = (l[None, :] > l[:, None]) | ((l[None, :] == l[:, None]) & (torch.arange(V)[None, :] < torch.arange(V)[:, None]))
    if mode == 0:
        return bigger.sum(dim=-1) < k
    p = torch.softmax(l, dim=-1)
    return (bigger.double() @ p) <= thres


def draw_row(rs: np.random.RandomState, V: int, kind: int) -> torch.Tensor:
    if kind == 0:
        x = rs.randn(V) * 3.0
    elif kind == 1:                               # one dominant entry
        x = rs.randn(V) * 3.0
        x[rs.randint(V)] += rs.uniform(6.0, 14.0)
    else:                                         # nearly flat
        x = rs.randn(V) * rs.choice([0.01, 0.05, 0.2])
    return torch.from_numpy(x.astype(np.float32))


def main():
    _install_shims()
    sys.path.insert(0, REF)
    from covomix.covomix_model.text2semantic import top_k, top_p               # reference
    save = {}
    for V, R in ROWS.items():
        sets = settings(V)
        rs = np.random.RandomState(1000 + V)
        rows, tried = [], 0
        while len(rows) < R:
            row = draw_row(rs, V, (0, 0, 1, 2)[len(rows) % 4])
            tried += 1
            if decided(row, sets):
                rows.append(row)
        logits = torch.stack(rows)
        masks = []
        for name, mode, k, thres in sets:
            if mode == 0:
                f = top_k(logits.clone(), thres=thres) if "thres" in name else top_k(logits.clone(), k=k)
            else:
                f = top_p(logits.clone(), thres=thres)
            m = f > float("-inf")
            want = torch.stack([fp64_mask(r, mode, k, thres) for r in logits])
            assert torch.equal(m, want), (V, name, int((m != want).sum()))
            assert bool(m.any(dim=-1).all())
            masks.append(m.numpy())
            print(V, name, "kept per row: min", int(m.sum(-1).min()), "max", int(m.sum(-1).max()))
        print(V, "rows", R, "drawn", tried)
        save[f"logits_{V}"] = logits.numpy()
        save[f"kept_{V}"] = np.stack(masks)                                     # [settings, R, V] bool
        save[f"mode_{V}"] = np.array([s[1] for s in sets], dtype=np.int32)
        save[f"k_{V}"] = np.array([s[2] for s in sets], dtype=np.int32)
        save[f"thres_{V}"] = np.array([s[3] for s in sets], dtype=np.float64)
        save[f"names_{V}"] = np.array([s[0] for s in sets])
    np.savez_compressed(OUT, **save)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 300 * 1024


if __name__ == "__main__":
    main()
