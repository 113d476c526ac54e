#!/usr/bin/env python3
"""Flow-matching validation loss of an acoustic checkpoint over a directory (CoVoMixModel.flow_matching_loss).

  python tools/eval_flow_loss.py --ckpt CKPT --mel_dir DIR --token_dir DIR [--cond_dir DIR] --json OUT [--seed 0] [--draws K]
                                 [--times t1,t2,...] [--precision f16x3|fp32|f16] [--max_rows N]

Files are paired by stem: `name.mel.npy` ([80, T], as the reference stores its mels) in mel_dir (and in cond_dir: the conditioning
mel, default the mel itself) with `name.semantic.npy` (int tokens [T] or [T, streams]) in token_dir.  Stems without a partner are
listed in OUT and on stderr, never skipped silently.  --draws K averages K independent draws (time, noise, mask: seeds seed,
seed + 1, ...) per utterance; --times evaluates every utterance at each given time (noise and mask still drawn) and reports the loss
per time - the loss-over-t curve of the checkpoint.  OUT receives the mean, the per-utterance losses, frames and times.

This is the reference's `valid_loss` with per-utterance semantics (no padded batch).  Figures from random-weight models say nothing
about quality: only the comparison of checkpoints of one model on one directory and one seed means something."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEL_SUFFIX, TOKEN_SUFFIX = ".mel.npy", ".semantic.npy"
NOTE = ("conditional-flow-matching loss, per-utterance masked mean (the reference's valid_loss at B = 1); figures from random-weight "
        "models say nothing about quality")


def times_arg(text: str) -> list:
    try:
        vals = [float(x) for x in text.split(",") if x.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--times {text!r}: comma-separated numbers") from None
    if not vals or not all(0.0 <= v <= 1.0 for v in vals):
        raise argparse.ArgumentTypeError(f"--times {text!r}: at least one time, each in [0, 1]")
    return vals


def positive(text: str) -> int:
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError(f"{text!r}: a positive integer")
    return v


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--mel_dir", required=True)
    ap.add_argument("--token_dir", required=True)
    ap.add_argument("--cond_dir", default=None, help="conditioning mels (default: the mels themselves)")
    ap.add_argument("--json", required=True, help="file the result is written to")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--draws", type=positive, default=1)
    ap.add_argument("--times", type=times_arg, default=None)
    ap.add_argument("--precision", choices=["f16x3", "fp32", "f16"], default=None)
    ap.add_argument("--max_rows", type=positive, default=8192)
    return ap


def stems(directory: str, suffix: str) -> dict:
    return {n[:-len(suffix)]: os.path.join(directory, n) for n in sorted(os.listdir(directory)) if n.endswith(suffix)}


def pair_by_stem(mel_dir: str, token_dir: str, cond_dir=None) -> tuple:
    """([(stem, mel path, token path, cond path or None)], {directory role: stems that lack a partner}), each sorted"""
    m, t = stems(mel_dir, MEL_SUFFIX), stems(token_dir, TOKEN_SUFFIX)
    c = stems(cond_dir, MEL_SUFFIX) if cond_dir else None
    both = set(m) & set(t) & (set(c) if c is not None else set(m))
    missing = dict(no_tokens=sorted(set(m) - set(t)), no_mel=sorted(set(t) - set(m)))
    if c is not None:
        missing["no_cond"] = sorted((set(m) & set(t)) - set(c))
        missing["cond_only"] = sorted(set(c) - set(m))
    return [(s, m[s], t[s], c[s] if c is not None else None) for s in sorted(both)], missing


def load(pairs) -> tuple:
    import numpy as np
    import torch

    def mel(p):
        a = torch.from_numpy(np.load(p).astype(np.float32))
        if a.dim() != 2:
            raise ValueError(f"{p}: a mel of shape {tuple(a.shape)} ([bins, T])")
        return a.t().contiguous()
    mels = [mel(p) for _, p, _, _ in pairs]
    toks = [torch.from_numpy(np.load(p).astype(np.int64)) for _, _, p, _ in pairs]
    conds = [mel(p) for _, _, _, p in pairs] if pairs and pairs[0][3] is not None else None
    return mels, toks, conds


def evaluate(model, pairs, seed: int = 0, draws: int = 1, times=None, max_rows: int = 8192) -> dict:
    """The result dict of the tool for a loaded model: without `times` K = draws calls at seeds seed + k; with them one such set per time."""
    mels, toks, conds = load(pairs)
    n = len(pairs)

    def mean_of(t):
        per = [0.0] * n
        for k in range(draws):
            r = model.flow_matching_loss(toks, mels, cond_mels=conds, times=None if t is None else [t] * n, seed=seed + k, max_rows=max_rows)
            per = [a + float(b) / draws for a, b in zip(per, r.per_utterance)]
            last = r
        return per, last
    out = dict(note=NOTE, seed=seed, draws=draws, utterances=[s for s, *_ in pairs], frames=[int(m.shape[0]) for m in mels])
    if times is None:
        per, last = mean_of(None)
        out.update(per_utterance=per, loss=sum(per) / n, times_of_last_draw=[float(x) for x in last.times])
    else:
        curve = []
        for t in times:
            per, _ = mean_of(t)
            curve.append(dict(time=t, loss=sum(per) / n, per_utterance=per))
        out.update(curve=curve, loss=sum(c["loss"] for c in curve) / len(curve))
    return out


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    sys.path.insert(0, ROOT)
    pairs, missing = pair_by_stem(args.mel_dir, args.token_dir, args.cond_dir)
    for role, names in missing.items():
        if names:
            print(f"{role}: {', '.join(names)}", file=sys.stderr)
    if not pairs:
        print("no utterance has all its files", file=sys.stderr)
        return 2
    from covomix_amd.conditional_model import CoVoMixModel
    kw = {} if args.precision is None else dict(precision=args.precision)
    model = CoVoMixModel.load_from_checkpoint(args.ckpt, **kw).eval().to("cuda")
    res = evaluate(model, pairs, args.seed, args.draws, args.times, args.max_rows)
    res["missing"] = missing
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
    print(f"{len(pairs)} utterances, flow-matching loss {res['loss']:.6f} ({NOTE})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
