#!/usr/bin/env python3
"""Step time of the text2semantic decode under the sampling controls, one JSON line per figure.

  python tools/t2s_sampling_bench.py steps  [--top-p 0.9] [--root OTHER_CHECKOUT]
      us per token step of the lock-step decode (generate_batch, ignore_eos, graph replay) for CoMix and CoSingle at 1 / 8 / 64
      slots; --top-p adds the same figure under the nucleus filter.  --root runs the package of another checkout (the parent
      commit, built there) so that parent and change can alternate in one session: run the command in turns, five rounds.
  python tools/t2s_sampling_bench.py guided
      64 guided CoSingle dialogues (cond_scale 1.5) that end at different steps (limits 100 ... 608, the eos ignored: the recipe of
      config5.decode_ragged) through generate_many(cond_scale=) on 32 slot pairs against lock-step guided batches of 32.
  python tools/t2s_sampling_bench.py steps --logprobs
      adds the step time with the log-prob epilogue on (return_logprobs=True: the scoring instantiation of the sampling kernel).
  python tools/t2s_sampling_bench.py score
      score_many of 64 x 608-token targets (forced dialogues) against generate_many of the same 64 x 608 steps, both on 64 slots.
  python tools/t2s_sampling_bench.py bestof
      dialogues per second of best-of 1 / 2 / 4 on 56 CoMix dialogues (608 steps each, the eos ignored: N * 56 decodes through 64 slots,
      log-probs on for N > 1, selection included).
  python tools/t2s_sampling_bench.py beam [--beam-size 10]
      us per beam step (generate_beam, graph replay) for CoMix and CoSingle with 1 and 6 utterances (10 and 60 slots at beam size 10).
      The sampled step at the same slot counts: `steps --slots 10,60` (with --root for the parent commit), in turns, five rounds.
  python tools/t2s_sampling_bench.py beamq [--beam-size 10]
      128 utterances that end at different steps (limits 100 ... 608: the set of config5.decode_ragged) for CoMix and CoSingle:
      generate_beam_many (continuously refilled groups) against generate_beam in lock-step waves of 64 // beam_size utterances, each wave
      as long as its longest utterance; in turns, five rounds, utterances per second.
  python tools/t2s_sampling_bench.py beamrules [--beam-size 10] [--root OTHER_CHECKOUT]
      beam search under the history rules (generate_beam(beam_rules=True): no 3-gram twice, minimum length 40, every utterance) against
      the plain beam chain, 60 slots: CoMix and CoSingle with 6 utterances, CoSingle under guidance (cond_scale 1.5) with 3.  The eos
      embedding row is zeroed (no hypothesis finishes: every call runs all its steps).  us per step over positions 256 .. 512 - the
      histories the rule kernels gather - = (wall time of 512 steps - wall time of 256 steps) / 256, sides alternating, five rounds, with the
      effective shader clock.  A checkout without beam_rules (--root, the parent commit) times the plain chain alone: run fresh
      processes of both in turns.
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["steps", "guided", "score", "bestof", "beam", "beamq", "beamrules"])
    ap.add_argument("--logprobs", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--top-p", type=float, default=None)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--tag", default="")
    ap.add_argument("--slots", default="1,8,64", help="steps: the slot counts")
    ap.add_argument("--beam-size", type=int, default=10)
    ap.add_argument("--utterances", default="1,6", help="beam: the utterance counts (a kernel trace wants one shape: --utterances 6)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import covomix_amd.synthetic as syn
    from covomix_amd.t2s import TextToSemanticDecoder
    dev = torch.device("cuda:0")
    shapes = {"comix": dict(two_output=True, dim=512, dim_target=1024), "cosingle": dict(two_output=False, dim=512, dim_target=512)}

    def model(name):
        sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(**shapes[name]), seed=0).items()}
        return TextToSemanticDecoder(sd, dev, max_length=max(args.steps, 608))

    def timed(fn):
        torch.cuda.synchronize(dev); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    g = torch.Generator().manual_seed(3)
    if args.what == "steps":
        for name in ("comix", "cosingle"):
            m = model(name)
            for slots in [int(x) for x in args.slots.split(",")]:
                srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(slots)]
                forms = (("default", {}),) + ((("top_p", dict(filter_logits_fn="top_p", filter_fn_kwargs={"thres": args.top_p})),) if args.top_p else ())
                forms += ((("logprobs", dict(return_logprobs=True)),) if args.logprobs else ())
                for label, kw in forms:
                    run = lambda: m.generate_batch(srcs, max_length=args.steps, ignore_eos=True, **kw)
                    run()                                                 # graph + buffers of the timed shape
                    t = min(timed(run) for _ in range(3))
                    print(json.dumps({"tag": args.tag, "model": name, "slots": slots, "filter": label, "steps": args.steps,
                                      "us_per_step": round(t / args.steps * 1e6, 1)}), flush=True)
    elif args.what == "beam":
        B = args.beam_size
        for name in ("comix", "cosingle"):
            m = model(name)
            for n in [int(x) for x in args.utterances.split(",")]:
                srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(n)]
                run = lambda: m.generate_beam(srcs, beam_size=B, max_length=args.steps)
                run()                                                     # graph + buffers of the timed shape
                t = min(timed(run) for _ in range(3))
                done = min(r["steps"] for r in m.last_beam)               # (an utterance whose hypotheses all finish ends early)
                print(json.dumps({"tag": args.tag, "model": name, "beam_size": B, "utterances": n, "slots": n * B, "steps": args.steps,
                                  "steps_of_the_shortest": done, "us_per_step": round(t / args.steps * 1e6, 1)}), flush=True)
    elif args.what == "beamrules":
        import inspect
        import statistics
        from covomix_amd import ops
        B = args.beam_size
        ruled = "beam_rules" in inspect.signature(TextToSemanticDecoder.generate_beam).parameters
        for name, scale, n in (("comix", 1.0, 60 // B), ("cosingle", 1.0, 60 // B), ("cosingle", 1.5, 60 // (2 * B))):
            sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(**shapes[name]), seed=0).items()}
            sd["semantic_token_emb.weight"][-1] = 0.0         # the eos logit is 0 at every step, far below the shortlists
            m = TextToSemanticDecoder(sd, dev, max_length=512)
            srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(n)]
            sides = [("plain", {})] + ([("rules", dict(beam_rules=True, no_repeat_ngram_size=3, min_length=40))] if ruled else [])
            run = lambda kw, steps: m.generate_beam(srcs, beam_size=B, max_length=steps, cond_scale=scale, **kw)
            for _, kw in sides:
                run(kw, 64)                                   # graph + buffers of the timed shape (min_length 40 fits)
            t = {k: [] for k, _ in sides}
            c0 = ops.clock_stamps()
            for r in range(5):
                for k, kw in (sides if r % 2 == 0 else sides[::-1]):
                    t256 = timed(lambda: run(kw, 256))
                    t512 = timed(lambda: run(kw, 512))
                    assert all(rec["steps"] == 512 for rec in m.last_beam), "a search ended early"
                    t[k].append((t512 - t256) / 256 * 1e6)
            clk = ops.clock_from_stamps(c0, ops.clock_stamps())
            out = {"tag": args.tag, "model": name, "cond_scale": scale, "beam_size": B, "utterances": n, "slots": n * B * (2 if scale > 1 else 1),
                   "positions": "256..512", "clock_mhz": round(clk["mhz"]) if clk else None}
            for k, _ in sides:
                out[k + "_us_per_step"] = [round(x, 1) for x in t[k]]
                out[k + "_median"] = round(statistics.median(t[k]), 1)
            if ruled:
                out["rules_minus_plain"] = round(out["rules_median"] - out["plain_median"], 1)
            print(json.dumps(out), flush=True)
    elif args.what == "beamq":
        B, n, tokens = args.beam_size, 128, 608
        per = 64 // B
        lims = torch.randint(100, tokens + 1, (n,), generator=g).tolist()
        srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(n)]
        for name in ("comix", "cosingle"):
            m = model(name)
            many = lambda l: m.generate_beam_many(srcs, beam_size=B, max_length=tokens, limits=l)
            waves = lambda: [m.generate_beam(srcs[w:w + per], beam_size=B, max_length=max(lims[w:w + per])) for w in range(0, n, per)]
            many([20] * n)                                                # graphs + buffers of the timed shapes
            m.generate_beam(srcs[:per], beam_size=B, max_length=20)
            m.generate_beam(srcs[:n % per or per], beam_size=B, max_length=20)
            for r in range(5):
                t_many = timed(lambda: many(lims))
                early = sum(1 for rec in m.last_beam if rec["status"] == 2)   # (ended before its limit: all hypotheses finished)
                t_waves = timed(waves)
                print(json.dumps({"tag": args.tag, "model": name, "round": r, "utterances": n, "beam_size": B, "groups": per,
                                  "useful_steps": sum(lims), "ended_by_eos": early, "refilled_s": round(t_many, 4),
                                  "waves_s": round(t_waves, 4), "refilled_utt_per_s": round(n / t_many, 2),
                                  "waves_utt_per_s": round(n / t_waves, 2), "refilled_vs_waves": round(t_waves / t_many, 3)}), flush=True)
    elif args.what == "score":
        for name in ("comix", "cosingle"):
            m = model(name)
            n, tokens, S, V = 64, 608, m.d["streams"], m.d["vocab"]
            srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(n)]
            tg = [torch.randint(0, V, (S, tokens), generator=g) for _ in range(n)]
            score = lambda: m.score_many(srcs, tg, slots=64)
            sample = lambda: m.generate_many(srcs, max_length=tokens, slots=64, ignore_eos=True)
            score(); sample()
            for r in range(5):
                t_score, t_sample = timed(score), timed(sample)
                print(json.dumps({"tag": args.tag, "model": name, "round": r, "dialogues": n, "tokens": tokens, "score_many_s": round(t_score, 4),
                                  "generate_many_s": round(t_sample, 4), "score_vs_generate": round(t_score / t_sample, 3)}), flush=True)
    elif args.what == "bestof":
        from covomix_amd.t2s import best_candidate, sequence_logprob
        m = model("comix")
        n, tokens, eos = 56, 608, m.d["vocab"] - 1
        srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(n)]

        def run(N):
            if N == 1:
                return m.generate_many(srcs, max_length=tokens, slots=64, ignore_eos=True)
            res = m.generate_many([s_ for s_ in srcs for _ in range(N)], max_length=tokens, slots=64, ignore_eos=True, return_logprobs=True)
            return [res[j * N + best_candidate([sequence_logprob(c[2], c[1], eos) for c in res[j * N:(j + 1) * N]])] for j in range(n)]
        for N in (1, 2, 4):
            run(N)
            t = min(timed(lambda: run(N)) for _ in range(3))
            print(json.dumps({"tag": args.tag, "best_of": N, "dialogues": n, "tokens": tokens, "seconds": round(t, 4),
                              "dialogues_per_s": round(n / t, 1)}), flush=True)
    else:
        m = model("cosingle")
        n, tokens, pairs = 64, 608, 32
        lims = torch.randint(100, tokens + 1, (n,), generator=g).tolist()
        srcs = [torch.randint(1, 30000, (1, 64), generator=g) for _ in range(n)]
        many = lambda l: m.generate_many(srcs, max_length=tokens, slots=2 * pairs, ignore_eos=True, limits=l, cond_scale=1.5)
        lock = lambda: [m.generate_batch(srcs[w:w + pairs], max_length=max(lims[w:w + pairs]), ignore_eos=True, cond_scale=1.5)
                        for w in range(0, n, pairs)]
        many([20] * n)
        m.generate_batch(srcs[:pairs], max_length=20, ignore_eos=True, cond_scale=1.5)
        for r in range(5):
            t_many, t_lock = timed(lambda: many(lims)), timed(lock)
            print(json.dumps({"tag": args.tag, "round": r, "dialogues": n, "slot_pairs": pairs, "useful_steps": sum(lims),
                              "continuous_s": round(t_many, 4), "lock_step_s": round(t_lock, 4),
                              "continuous_vs_lock_step": round(t_lock / t_many, 3)}), flush=True)


if __name__ == "__main__":
    main()
