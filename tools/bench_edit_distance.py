#!/usr/bin/env python3
"""Dev: what the edit-distance call costs (ops.edit_distance / cvx_edit_distance_i64) and what consensus selection adds to best-of-N.

  python tools/bench_edit_distance.py kernel
      One call for 64 utterances x 8 candidates x 2 streams of 400 - 600 tokens (the 3,584 unordered pairs of t2s.consensus_pairs;
      candidates of an utterance are mutations of one base sequence over 500 symbols): kernel time (device events around the entry point,
      tables and tokens already on the device), wall time of ops.edit_distance from host tensors to the host result (pooled upload,
      launch, download), the numpy restatement (tests/edit_distance_restated.py) of the same pairs on 16 worker processes, and one pair
      at 4096 x 4096.  ROUNDS (20) timed rounds after WARM (3); median (min .. max) and the effective shader clock.  The GPU result is
      checked against the restatement before anything is timed.
  python tools/bench_edit_distance.py select --select mbr|logprob [--root OTHER_CHECKOUT]
      One synthesis_sample_text2semantic(best_of=8) call of 64 utterances on the synthetic CoMix model (two streams, max_length 600:
      512 decodes through 64 slots), seeded draws: wall seconds of ROUNDS (3) calls after one untimed call, and under mbr the part of
      each call spent choosing (scores, risks, the edit-distance call).  Meant for fresh processes in turns: mbr, logprob and - with
      --root, the parent commit built there - the parent's logprob.
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


def consensus_set(utterances=64, candidates=8, streams=2, seed=0):
    """(sequences, pairs): item (u, c, s) at (u * candidates + c) * streams + s"""
    rng = np.random.RandomState(seed)
    seqs, pairs = [], []
    for u in range(utterances):
        bases = [rng.randint(0, 500, size=600) for _ in range(streams)]
        at = len(seqs)
        for c in range(candidates):
            for s in range(streams):
                x = bases[s][:rng.randint(400, 601)].copy()
                x[rng.rand(x.size) < 0.1] = rng.randint(0, 500)
                seqs.append(np.delete(x, np.nonzero(rng.rand(x.size) < 0.03)[0])[:600])
        pairs += [(at + c * streams + s, at + c2 * streams + s) for c in range(candidates) for c2 in range(c + 1, candidates)
                  for s in range(streams)]
    return seqs, pairs


def _restated_chunk(job):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edit_distance_restated as rs
    seqs, pairs = job
    return [rs.distance(seqs[i], seqs[j]) for i, j in pairs]


def kernel():
    import multiprocessing as mp
    rounds, warm = int(os.environ.get("ROUNDS", "20")), int(os.environ.get("WARM", "3"))
    seqs, pairs = consensus_set()
    lens = [len(s) for s in seqs]
    cells = sum(lens[i] * lens[j] for i, j in pairs)
    # the restatement first, before this process opens the GPU: 16 workers that never touch it
    with mp.get_context("spawn").Pool(16) as pool:
        chunks = [pairs[k::64] for k in range(64)]
        pool.map(_restated_chunk, [(seqs, c[:2]) for c in chunks[:16]])          # workers started and imports done
        t_np = []
        for _ in range(3):
            t0 = time.perf_counter()
            parts = pool.map(_restated_chunk, [(seqs, c) for c in chunks])
            t_np.append((time.perf_counter() - t0) * 1e3)
    want = np.zeros(len(pairs), dtype=np.int32)
    for k, part in enumerate(parts):
        want[k::64] = part
    import torch
    sys.path.insert(0, ROOT)
    from covomix_amd import _lib, ops
    assert torch.cuda.is_available(), "bench_edit_distance.py measures on the GPU"
    dev = torch.device("cuda:0")
    host = [torch.from_numpy(s.astype(np.int64)) for s in seqs]
    got = ops.edit_distance(host, pairs)
    assert np.array_equal(got.numpy(), want), "the kernel differs from the restatement"
    lib = _lib.load()
    items, prs = ops.edit_distance_tables(lens, pairs)
    tok_d, items_d, prs_d = torch.cat(host).to(dev), items.to(dev), prs.to(dev)
    out = torch.empty(len(pairs), dtype=torch.int32, device=dev)

    def launch(tok, it, it_d, pr, pr_d, o):
        _lib.check(lib.cvx_edit_distance_i64(tok.data_ptr(), tok.numel(), it.data_ptr(), it_d.data_ptr(), it.shape[0], pr.data_ptr(),
                                             pr_d.data_ptr(), pr.shape[0], o.data_ptr(), ops._stream()), "cvx_edit_distance_i64")

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
    c0 = ops.clock_stamps()
    t_k = events(lambda: launch(tok_d, items, items_d, prs, prs_d, out))
    assert np.array_equal(out.cpu().numpy(), want)
    t_w = []
    for r in range(warm + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.edit_distance(host, pairs)
        if r >= warm:
            t_w.append((time.perf_counter() - t0) * 1e3)
    rng = np.random.RandomState(1)
    big = [torch.from_numpy(rng.randint(0, 500, size=4096).astype(np.int64)) for _ in range(2)]
    it1, pr1 = ops.edit_distance_tables([4096, 4096], [(0, 1)])
    big_d, it1_d, pr1_d, out1 = torch.cat(big).to(dev), it1.to(dev), pr1.to(dev), torch.empty(1, dtype=torch.int32, device=dev)
    t_1 = events(lambda: launch(big_d, it1, it1_d, pr1, pr1_d, out1))
    clk = ops.clock_from_stamps(c0, ops.clock_stamps())
    say({"what": "consensus set", "device": torch.cuda.get_device_name(0), "sequences": len(seqs), "pairs": len(pairs),
         "tokens_per_sequence": f"{min(lens)} .. {max(lens)}", "cells": cells, "rounds": rounds,
         "kernel_ms": med(t_k), "gcells_per_s": round(cells / statistics.median(t_k) / 1e6, 1),
         "ops_edit_distance_wall_ms": med(t_w), "numpy_16_processes_ms": med(t_np),
         "clock_mhz": round(clk["mhz"]) if clk else None})
    say({"what": "one pair 4096 x 4096", "kernel_ms": med(t_1), "distance": int(out1.cpu()[0]),
         "gcells_per_s": round(4096 * 4096 / statistics.median(t_1) / 1e6, 2)})


def select(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel
    rounds = int(os.environ.get("ROUNDS", "3"))
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(two_output=True, dim=512, dim_target=1024), seed=0).items()}
    m = CoVoMixModel(sd, hparams={"text2semantic": True}).eval().to(dev)
    g = torch.Generator().manual_seed(3)
    ids = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(64)]
    kw = dict(best_of=8, max_length=600, return_logprobs=True)
    if args.select == "mbr":
        kw["best_of_select"] = "mbr"
    choosing = []
    if hasattr(CoVoMixModel, "_select_candidates"):
        real = CoVoMixModel._select_candidates

        def timed_select(*a):
            t0 = time.perf_counter()
            r = real(*a)
            choosing.append(time.perf_counter() - t0)
            return r
        CoVoMixModel._select_candidates = staticmethod(timed_select)

    def run(seed):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = m.synthesis_sample_text2semantic(ids, generator=torch.Generator(device=dev).manual_seed(seed), **kw)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, res
    run(0)
    choosing.clear()
    t, lens = [], []
    for r in range(rounds):
        dt, res = run(1 + r)
        t.append(dt)
        lens += [int(x[1].shape[1]) for x in res]
    say({"what": "best_of 8 x 64 utterances, CoMix", "tag": args.tag, "select": args.select, "seconds": [round(x, 4) for x in t],
         "median_s": round(statistics.median(t), 4), "choosing_s": [round(x, 4) for x in choosing],
         "chosen_lengths": f"{min(lens)} .. {max(lens)}"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "select"])
    ap.add_argument("--select", choices=["logprob", "mbr"], default="logprob")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    kernel() if args.what == "kernel" else select(args)


if __name__ == "__main__":
    main()
