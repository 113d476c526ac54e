#!/usr/bin/env python3
"""Mel-cepstral distortion between the files of two directories (covomix_amd.metrics.mel_cepstral_distortion).

  python tools/eval_mel.py --pred_dir DIR --ref_dir DIR --json OUT [--n_coef 13] [--align dtw|none]

Files are paired by stem: `name.wav` (any rate and sample type; through mel.extract_mel_many) or `name.mel.npy` ([80, T], as the
reference stores its mels); a stem may be a wav on one side and a mel on the other.  OUT receives per pair the MCD in dB, the length of
the alignment path and the frames of both sides, the mean over the pairs, and the stems that have no partner (listed, never skipped
silently).  All cepstra come from one GEMM call and all alignments from one launch of the DTW kernel.

The MCD is THIS PROJECT'S DEFINITION (cepstra 1 ... n_coef of the orthonormal DCT-II of the 80-bin natural-log mel): comparable only
within it, not with published figures.  Figures from random-weight models say nothing about audio quality."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIXES = (".mel.npy", ".wav")
NOTE = ("MCD in this project's definition (DCT-II cepstra 1..n_coef of the 80-bin natural-log mel): comparable only within it; "
        "figures from random-weight models say nothing about audio quality")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pred_dir", required=True)
    ap.add_argument("--ref_dir", required=True)
    ap.add_argument("--json", required=True, help="file the result is written to")
    ap.add_argument("--n_coef", type=int, default=13)
    ap.add_argument("--align", choices=["dtw", "none"], default="dtw")
    return ap


def stems(directory: str) -> dict:
    """{stem: path} of the .wav and .mel.npy files of a directory; a stem present in both forms keeps its mel"""
    found = {}
    for name in sorted(os.listdir(directory)):
        for suf in SUFFIXES:
            if name.endswith(suf) and name[:-len(suf)] not in found:
                found[name[:-len(suf)]] = os.path.join(directory, name)
    return found


def pair_by_stem(pred_dir: str, ref_dir: str) -> tuple:
    """([(stem, pred path, ref path)], stems only in pred_dir, stems only in ref_dir), each sorted"""
    p, r = stems(pred_dir), stems(ref_dir)
    both = sorted(set(p) & set(r))
    return [(s, p[s], r[s]) for s in both], sorted(set(p) - set(r)), sorted(set(r) - set(p))


def load_mels(paths) -> list:
    """[T, 80] float32 mels of the paths: .mel.npy files are read, all wavs go through ONE mel.extract_mel_many call"""
    import numpy as np
    import torch
    from covomix_amd import mel
    wavs = [p for p in paths if p.endswith(".wav")]
    from_wav = dict(zip(wavs, mel.extract_mel_many(wavs))) if wavs else {}
    out = []
    for p in paths:
        m = from_wav[p] if p in from_wav else torch.from_numpy(np.load(p).astype(np.float32))
        if m.dim() != 2 or m.shape[0] != 80:
            raise ValueError(f"{p}: a mel of shape {tuple(m.shape)} ([80, T])")
        out.append(m.t().contiguous())
    return out


def evaluate(pred_dir: str, ref_dir: str, n_coef: int = 13, align: str = "dtw") -> dict:
    from covomix_amd.metrics import mel_cepstral_distortion
    pairs, only_pred, only_ref = pair_by_stem(pred_dir, ref_dir)
    rows = []
    if pairs:
        mels = load_mels([p for _, p, _ in pairs] + [r for _, _, r in pairs])
        pred, ref = mels[:len(pairs)], mels[len(pairs):]
        mcd, steps = mel_cepstral_distortion(pred, ref, n_coef=n_coef, align=align)
        rows = [dict(stem=s, mcd_db=float(d), steps=int(n), pred_frames=a.shape[0], ref_frames=b.shape[0])
                for (s, _, _), d, n, a, b in zip(pairs, mcd, steps, pred, ref)]
    good = [r["mcd_db"] for r in rows if not math.isnan(r["mcd_db"])]
    return dict(note=NOTE, n_coef=n_coef, align=align, pairs=rows, mean_mcd_db=sum(good) / len(good) if good else None,
                missing_in_ref_dir=only_pred, missing_in_pred_dir=only_ref)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    sys.path.insert(0, ROOT)
    res = evaluate(args.pred_dir, args.ref_dir, args.n_coef, args.align)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
    for side, names in (("ref_dir", res["missing_in_ref_dir"]), ("pred_dir", res["missing_in_pred_dir"])):
        if names:
            print(f"no partner in {side}: {', '.join(names)}", file=sys.stderr)
    print(f"{len(res['pairs'])} pairs, mean MCD {res['mean_mcd_db']} dB ({NOTE})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
