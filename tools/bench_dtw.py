#!/usr/bin/env python3
"""Dev: what the DTW call costs (ops.dtw / cvx_dtw_f32, csrc/dtw.hip).

  python tools/bench_dtw.py [--pairs 64,512] [--dims 13,80] [--no-numpy]
      For every (pairs, D): that many pairs of 800 - 1200 x 800 - 1200 frames of D features (a test set of generated against target
      cepstra or mels): kernel time (device events around the entry point, frames and tables already on the device) and wall time of
      ops.dtw from host tensors to the host result (pooled upload, launch, download).  For the smallest set of every D also the numpy
      restatement (tests/dtw_restated.py) of the same pairs on 16 worker processes, against which the GPU result is checked bit for bit
      before anything is timed.  Then one pair at 4096 x 4096 for every D.  ROUNDS (20) timed rounds after WARM (3); median
      (min .. max) and the effective shader clock beside every figure.  Meant to be run in a few fresh processes.
One JSON line per figure; OUT=file appends them there."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def say(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "a") as f:
            f.write(line + "\n")


def med(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def test_set(n_pairs, dim, seed=0):
    """(features, pairs): pair p = (2 p, 2 p + 1); the second item is a time-warped, noisy copy of the first"""
    rng = np.random.RandomState(seed + dim)
    feats = []
    for _ in range(n_pairs):
        a = rng.standard_normal((rng.randint(800, 1201), dim)).astype(np.float32)
        at = np.sort(rng.randint(0, a.shape[0], size=rng.randint(800, 1201)))
        feats += [a, (a[at] + 0.3 * rng.standard_normal((at.size, dim))).astype(np.float32)]
    return feats, [(2 * p, 2 * p + 1) for p in range(n_pairs)]


def _restated_chunk(job):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dtw_restated as rs
    return [rs.dtw(a, b) for a, b in job]


def main():
    import multiprocessing as mp
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="64,512")
    ap.add_argument("--dims", default="13,80")
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    rounds, warm = int(os.environ.get("ROUNDS", "20")), int(os.environ.get("WARM", "3"))
    sizes, dims = sorted(int(x) for x in args.pairs.split(",")), [int(x) for x in args.dims.split(",")]
    sets = {(n, d): test_set(n, d) for n in sizes for d in dims}
    # the restatement first, before this process opens the GPU: 16 workers that never touch it
    restated = {}
    if not args.no_numpy:
        with mp.get_context("spawn").Pool(16) as pool:
            pool.map(_restated_chunk, [[(np.zeros((2, 2), np.float32),) * 2]] * 16)          # workers started and imports done
            for d in dims:
                feats, pairs = sets[(sizes[0], d)]
                jobs = [[(feats[i], feats[j]) for i, j in pairs[k::16]] for k in range(16)]
                t0 = time.perf_counter()
                parts = pool.map(_restated_chunk, jobs)
                ms = (time.perf_counter() - t0) * 1e3
                want = [None] * len(pairs)
                for k, part in enumerate(parts):
                    want[k::16] = part
                restated[d] = (want, ms)
    import torch
    sys.path.insert(0, ROOT)
    from covomix_amd import _lib, ops
    assert torch.cuda.is_available(), "bench_dtw.py measures on the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def on_device(feats, pairs):
        d = feats[0].shape[1]
        ld = (d + 3) // 4 * 4
        items, prs = ops.dtw_tables([f.shape[0] for f in feats], pairs)
        pool = torch.zeros(int(items[:, 1].sum()), ld)
        pool[:, :d] = torch.from_numpy(np.concatenate(feats))
        out = torch.empty(2 * len(pairs), dtype=torch.int32, device=dev)
        return pool.to(dev), d, items, items.to(dev), prs, prs.to(dev), out

    def launch(pool, d, it, it_d, pr, pr_d, out):
        _lib.check(lib.cvx_dtw_f32(pool.data_ptr(), pool.shape[0], pool.shape[1], d, it.data_ptr(), it_d.data_ptr(), it.shape[0], pr.data_ptr(),
                                   pr_d.data_ptr(), pr.shape[0], out.data_ptr(), out.data_ptr() + 4 * pr.shape[0], ops._stream()), "cvx_dtw_f32")

    def events(fn):
        t = []
        for r in range(warm + rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if r >= warm:
                t.append(e0.elapsed_time(e1))
        return t

    for (n, d), (feats, pairs) in sorted(sets.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        host = [torch.from_numpy(f) for f in feats]
        cost, steps = ops.dtw(host, pairs)
        if d in restated and n == sizes[0]:
            want = restated[d][0]
            assert all(c.numpy().tobytes() == w[0].tobytes() and int(s) == w[1] for c, s, w in zip(cost, steps, want)), \
                "the kernel differs from the restatement"
        ops_args = on_device(feats, pairs)
        cells = sum(feats[i].shape[0] * feats[j].shape[0] for i, j in pairs)
        c0 = ops.clock_stamps()
        t_k = events(lambda: launch(*ops_args))
        clk = ops.clock_from_stamps(c0, ops.clock_stamps())
        t_w = []
        for r in range(warm + rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.dtw(host, pairs)
            if r >= warm:
                t_w.append((time.perf_counter() - t0) * 1e3)
        rec = {"what": "test set", "device": torch.cuda.get_device_name(0), "pairs": n, "dim": d, "frames": "800 .. 1200", "cells": cells,
               "rounds": rounds, "kernel_ms": med(t_k), "gcells_per_s": round(cells / statistics.median(t_k) / 1e6, 2),
               "ops_dtw_wall_ms": med(t_w), "mean_steps": round(float(steps.double().mean()), 1),
               "clock_mhz": round(clk["mhz"]) if clk else None}
        if d in restated and n == sizes[0]:
            rec["numpy_16_processes_ms"] = round(restated[d][1], 1)
            rec["checked_against_the_restatement"] = True
        say(rec)
    for d in dims:
        rng = np.random.RandomState(1)
        big = [rng.standard_normal((4096, d)).astype(np.float32) for _ in range(2)]
        ops_args = on_device(big, [(0, 1)])
        c0 = ops.clock_stamps()
        t_1 = events(lambda: launch(*ops_args))
        clk = ops.clock_from_stamps(c0, ops.clock_stamps())
        out = ops_args[-1].cpu()
        nsteps = {13: 4 * (4096 + 255), 80: 16 * (4096 + 255)}.get(d)       # bands x (columns + threads - 1)
        rec = {"what": "one pair 4096 x 4096", "dim": d, "kernel_ms": med(t_1), "cost": float(out[:1].view(torch.float32)[0]), "steps": int(out[1]),
               "gcells_per_s": round(4096 * 4096 / statistics.median(t_1) / 1e6, 3), "clock_mhz": round(clk["mhz"]) if clk else None}
        if nsteps and clk:
            rec["pipeline_steps"] = nsteps
            rec["cycles_per_pipeline_step"] = round(statistics.median(t_1) * 1e-3 * clk["mhz"] * 1e6 / nsteps)
        say(rec)


if __name__ == "__main__":
    main()
