#!/usr/bin/env python3
"""The text2semantic prefill pass against the step chain, one JSON line per figure, on the full-size synthetic
CoSingle and CoMix (the models config5.py builds).

  python tools/t2s_prefill_bench.py score [--root OTHER_CHECKOUT] [--tag T]
      wall time of score_many for n in {1, 8, 64} utterances x L in {128, 600} tokens: the step chain (prefill=False) and, where the
      checkout has the switch, the pass (prefill=True) with the share of its time spent in the two attention launches of every layer
      (events around ops.t2s_prefill_attention).  Best of three after a warm-up call, with the effective shader clock of the process.
  python tools/t2s_prefill_bench.py continue [--root OTHER_CHECKOUT] [--tag T]
      a 300-token prefix plus 100 sampled steps (the eos ignored) for 1, 8 and 32 utterances on 64 slots: generate_many(prefixes=) with
      the prefix re-fed step by step and, where the checkout has the switch, through the pass (prefill=True).
  python tools/t2s_prefill_bench.py short [--tag T]
      where the windows of prefill=True lose: 128 utterances with a SHORT prefix (4, 16 or 64 tokens) that end at different steps (100 ..
      400 sampled steps, the eos ignored) through 64 slots - the step chain refills a slot the moment its utterance ends, the pass runs
      two windows of 64 utterances, each as long as its longest one.
--root runs the package of another checkout (the parent commit, built there), which times the step chain alone: run fresh processes
of both checkouts in turns (this tool is one process, one checkout)."""
import argparse
import inspect
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["score", "continue", "short"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="")
    ap.add_argument("--models", default="cosingle,comix")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import covomix_amd.synthetic as syn
    from covomix_amd import ops
    from covomix_amd.t2s import TextToSemanticDecoder
    dev = torch.device("cuda:0")
    shapes = {"comix": dict(two_output=True, dim=512, dim_target=1024), "cosingle": dict(two_output=False, dim=512, dim_target=512)}
    has_pass = "prefill" in inspect.signature(TextToSemanticDecoder.score_many).parameters

    def timed(fn):
        torch.cuda.synchronize(dev); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def best(fn):
        fn()                                                  # graphs and buffers of the timed shape
        return min(timed(fn) for _ in range(3))

    att = {"events": []}
    if has_pass:
        real = ops.t2s_prefill_attention

        def spied(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = real(*a, **kw); e1.record()
            att["events"].append((e0, e1))
            return out

    def attention_ms(fn):
        """(wall seconds of fn, milliseconds of it inside ops.t2s_prefill_attention) - a run of its own, not a timed one"""
        ops.t2s_prefill_attention = spied
        try:
            att["events"] = []
            t = timed(fn)
            return t, sum(a.elapsed_time(b) for a, b in att["events"])
        finally:
            ops.t2s_prefill_attention = real

    g = torch.Generator().manual_seed(3)
    c0 = ops.clock_stamps()
    for name in args.models.split(","):
        sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(**shapes[name]), seed=0).items()}
        m = TextToSemanticDecoder(sd, dev, max_length=608)
        S, V = m.d["streams"], m.d["vocab"]
        if args.what == "score":
            for n in (1, 8, 64):
                for L in (128, 600):
                    srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(n)]
                    tg = [torch.randint(0, V - 1, (S, L), generator=g) for _ in range(n)]
                    out = {"tag": args.tag, "what": "score", "model": name, "utterances": n, "tokens": L,
                           "steps_ms": round(best(lambda: m.score_many(srcs, tg, slots=64)) * 1e3, 3)}
                    if has_pass:
                        run = lambda: m.score_many(srcs, tg, prefill=True)
                        out["pass_ms"] = round(best(run) * 1e3, 3)
                        t, a_ms = attention_ms(run)
                        out["pass_attention_share"] = round(a_ms / (t * 1e3), 3)
                        out["steps_vs_pass"] = round(out["steps_ms"] / out["pass_ms"], 2)
                    print(json.dumps(out), flush=True)
        elif args.what == "short":
            n = 128
            srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(n)]
            steps = torch.randint(100, 401, (n,), generator=g).tolist()
            for P in (4, 16, 64):
                pre = [torch.randint(0, V - 1, (S, P), generator=g) for _ in range(n)]
                kw = dict(max_length=P + 400, slots=64, ignore_eos=True, prefixes=pre, limits=[P + x for x in steps])
                out = {"tag": args.tag, "what": "short", "model": name, "utterances": n, "prefix": P, "sampled_steps": sum(steps),
                       "steps_ms": round(best(lambda: m.generate_many(srcs, **kw)) * 1e3, 3),
                       "pass_ms": round(best(lambda: m.generate_many(srcs, prefill=True, **kw)) * 1e3, 3)}
                out["steps_vs_pass"] = round(out["steps_ms"] / out["pass_ms"], 2)
                print(json.dumps(out), flush=True)
        else:
            P, STEPS = 300, 100
            for n in (1, 8, 32):
                srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(n)]
                pre = [torch.randint(0, V - 1, (S, P), generator=g) for _ in range(n)]
                kw = dict(max_length=P + STEPS, slots=64, ignore_eos=True, prefixes=pre)
                out = {"tag": args.tag, "what": "continue", "model": name, "utterances": n, "prefix": P, "sampled_steps": STEPS,
                       "steps_ms": round(best(lambda: m.generate_many(srcs, **kw)) * 1e3, 3)}
                if has_pass:
                    out["pass_ms"] = round(best(lambda: m.generate_many(srcs, prefill=True, **kw)) * 1e3, 3)
                    out["steps_vs_pass"] = round(out["steps_ms"] / out["pass_ms"], 2)
                print(json.dumps(out), flush=True)
        del m
    clk = ops.clock_from_stamps(c0, ops.clock_stamps())
    print(json.dumps({"tag": args.tag, "what": args.what, "clock_mhz": round(clk["mhz"]) if clk else None}), flush=True)


if __name__ == "__main__":
    main()
