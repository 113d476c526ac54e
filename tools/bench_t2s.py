#!/usr/bin/env python3
"""Dev: text2semantic decode rate (us/step, tokens/s) for the CoSingle / CoMix configurations with recipe weights at decode batches
1 ... 64: encoder once, then N token steps through the graph-replayed decode loop (eos ignored so that the step count is fixed), then
the continuous-batching path (generate_many) on utterances that END at different steps against the lock-step batch.
Also prints the weight bytes a token step has to stream (the HBM/MALL roofline of a batch-1 decode).
    TOKENS=512 SIDE=0 BATCHES=1,8,16,32,64 python tools/bench_t2s.py [comix|cosingle]
PER=1: instead, the per-dialogue sampling path (cvx_t2s_decode_steps_per_dialogue) against the scalar path on the full-size CoMix model,
64 slots, eos ignored, STEPS (256) steps of graph replays: A = the scalar chain, B = every table row holding the same (default) setting,
C = rows alternating top-k and top-p across the slots; A / B / C interleaved REPEATS (5) times in one process -> us per step, min /
median / max of each, and the effective shader clock over the rounds (ops.clock_stamps).
    PER=1 STEPS=256 REPEATS=5 OUT=profile.txt python tools/bench_t2s.py
MIXED=1: the mixed slot pool (cvx_t2s_decode_steps_mixed) on the full-size CoSingle (one-output) model.  (a) us per step at 8 / 32 / 64
slots, eos ignored, all records unguided: A = cvx_t2s_decode_steps_per_dialogue behind a queue, B = the mixed entry (one launch more per
step: the scheduler), interleaved REPEATS times.  (b) 32 guided + 64 unguided utterances with step limits spread over 100..608, 64 slots:
one generate_many(mixed_guidance=True) call against the two calls of the default path (guided, then unguided), wall time, interleaved.
    MIXED=1 STEPS=256 REPEATS=5 OUT=profile.txt python tools/bench_t2s.py
BEAM=1: beam search (generate_beam, graph replay) on the full-size CoSingle model with the eos embedding row zeroed - its logit is then 0
at every step, far below the shortlists, so no hypothesis finishes and every call runs STEPS (256) steps (checked).  us per beam step = the
wall time of the call / STEPS (the encoder pass, the arming copies and the back-track included, the same for every side).  PARTS (a,b,c):
(a) unguided, beam size 10 x 6 utterances = 60 slots; (b) guided (scale 1.5), beam size 10 x 3 utterances = the same 60 slots - (a) and (b)
interleaved REPEATS times in one process; (c) generate_beam_many(cond_scale=1.5) against generate_beam(cond_scale=1.5) in lock-step waves of
3 utterances (each wave to its longest limit) on 24 utterances with step limits 100..608.  PARTS=a runs on a commit without guided beams
too: fresh processes of two commits, alternating, compare them.
    BEAM=1 PARTS=a,b,c STEPS=256 REPEATS=5 OUT=profile.txt python tools/bench_t2s.py
RULES=1: the history rules (cvx_t2s_decode_steps_rules) on the full-size CoMix and CoSingle models at 8 and 64 slots, slot b decoding
dialogue b without a queue.  Every run decodes WARM (256) untimed steps - the histories the rules scan - and then STEPS (256) timed ones, so a
timed step sees a history of WARM .. WARM + STEPS tokens per stream.  SIDES (D,A,B): D = the default chain (cvx_t2s_decode_steps), A = the
per-dialogue chain with one (default) setting in every row, B = the rules chain on the same settings with an active rule set in every row
(penalty 1.3 over the last 64 tokens, no 3-gram twice, minimum length beyond the run); interleaved REPEATS times -> us per step, min / median
/ max, and the effective shader clock.  SIDES=D,A uses nothing a commit without the rules lacks: fresh processes of two commits, alternating,
compare them (OUT is appended to).
    RULES=1 SIDES=D,A,B STEPS=256 WARM=256 REPEATS=5 OUT=profile.txt python tools/bench_t2s.py"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import covomix_amd.synthetic as syn
from covomix_amd.t2s import TextToSemanticDecoder, CHUNK
from covomix_amd import ops
dev = torch.device("cuda:0")
N = int(os.environ.get("TOKENS", "512"))
BATCHES = [int(x) for x in os.environ.get("BATCHES", "1,2,4,8,16,32,64").split(",")]
which = sys.argv[1:] or ["cosingle", "comix"]
if os.environ.get("SIDE", "0") == "1":          # on the 32-CU side stream of the CU partition (pipeline.py)
    torch.cuda.set_stream(ops.cu_partition(dev).side)
    print("on the side stream of the CU partition:", ops.stream_cus(), "CUs")


def per_dialogue_ab():
    """A / B / C interleaved, one process (see the module docstring)"""
    import statistics
    steps, reps, nb = int(os.environ.get("STEPS", "256")), int(os.environ.get("REPEATS", "5")), 64
    sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(two_output=True, dim=512, dim_target=1024), seed=0).items()}
    m = TextToSemanticDecoder(sd, dev, max_length=2048)
    from covomix_amd.t2s import check_settings, settings_rows
    g = torch.Generator().manual_seed(3)
    srcs = [torch.randint(1, 30000, (1, 48), generator=g) for _ in range(nb)]
    V, S = m.d["vocab"], m.d["streams"]
    same = [{} for _ in range(nb)]
    mixed = [{} if j % 2 == 0 else {"filter_logits_fn": "top_p", "filter_fn_kwargs": {"thres": 0.9}} for j in range(nb)]
    rows = lambda st: settings_rows(check_settings(st, nb, V, S)).to(dev)
    sides = (("A scalar path", None), ("B per-dialogue, one setting", rows(same)), ("C per-dialogue, top-k / top-p alternating", rows(mixed)))
    m._ensure(nb, nb, steps)
    m._graph(1.0, nb)
    m._graph(1.0, nb, per=True)
    rec = m._slot_records(m._contexts(srcs)).to(dev)
    m.buf["uniforms"].uniform_(1e-6, 1 - 1e-6)
    start = m.start[None, :].expand(nb, -1)
    def run(table):                                      # slot b decodes dialogue b from position 0, no queue: `steps` steps whatever is sampled
        m.buf["x"][:nb].copy_(start)
        m.buf["state"].copy_(rec)
        if table is not None:
            m.buf["per"][:nb].copy_(table)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(steps // CHUNK):
            m._run_chunk(1.0, nb, per=table is not None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6, m.buf["tokens"][:nb, :, :steps].clone()

    ref = {}
    for name, st in sides:                               # warm-up: graphs and buffers of every timed shape; and the results must agree
        ref[name] = run(st)[1]
    assert torch.equal(ref[sides[0][0]], ref[sides[1][0]]), "B decodes other tokens than A"
    c0 = ops.clock_stamps()
    t = {name: [] for name, _ in sides}
    for _ in range(reps):
        for name, st in sides:
            t[name].append(run(st)[0])
    clk = ops.clock_from_stamps(c0, ops.clock_stamps())
    lines = [f"text2semantic, full-size CoMix (synthetic weights), {nb} slots, ignore_eos, {steps} steps (slot b decodes dialogue b, eos ignored): "
             f"{steps // CHUNK} graph replays of {CHUNK} steps between two synchronisations / {steps}; {reps} rounds A B C A B C ...",
             f"device: {torch.cuda.get_device_name(0)}; effective shader clock over the timed rounds (cycle counter / real time, "
             f"{clk.get('cus', 0)} CUs): " + (f"{clk['mhz']:.0f} MHz" if clk else "not reported")]
    for name, _ in sides:
        v = sorted(t[name])
        lines.append(f"  {name:45s} us/step  min {v[0]:8.1f}  median {statistics.median(v):8.1f}  max {v[-1]:8.1f}   all {[round(x, 1) for x in t[name]]}")
    a, b_ = sorted(t[sides[0][0]]), sorted(t[sides[1][0]])
    spread = a[-1] - a[0]
    lines.append(f"  A's own spread {spread:.1f} us; B median - A median = {statistics.median(b_) - statistics.median(a):+.1f} us "
                 f"({'inside' if a[0] - spread <= statistics.median(b_) <= a[-1] + spread else 'OUTSIDE'} A's min..max widened by that spread)")
    print("\n".join(lines), flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")


def mixed_ab():
    """(a) and (b) of MIXED=1 (see the module docstring)"""
    import statistics
    from covomix_amd.t2s import SR, check_settings, settings_rows
    steps, reps = int(os.environ.get("STEPS", "256")), int(os.environ.get("REPEATS", "5"))
    sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(two_output=False, dim=512, dim_target=512), seed=0).items()}
    m = TextToSemanticDecoder(sd, dev, max_length=2048)
    V, S = m.d["vocab"], m.d["streams"]
    g = torch.Generator().manual_seed(3)
    med = statistics.median
    lines = [f"text2semantic, full-size CoSingle (synthetic weights), device: {torch.cuda.get_device_name(0)}",
             f"(a) us per step, {steps} steps = {steps // CHUNK} graph replays of {CHUNK} steps between two synchronisations, eos ignored, every "
             f"record unguided, one record per slot behind a queue; {reps} rounds A B A B ...: A = cvx_t2s_decode_steps_per_dialogue (34 launches "
             "per step), B = cvx_t2s_decode_steps_mixed (35: + the scheduler)"]
    for nb in (8, 32, 64):
        srcs = [torch.randint(1, 30000, (1, 48), generator=g) for _ in range(nb)]
        m._ensure(nb, nb, steps)
        m._graph(1.0, nb, 1.0, True, None, nb, False, True)
        m._graph(1.0, nb, 1.0, True, None, nb, False, True, 0)
        ctx = m._contexts(srcs)
        m.buf["uniforms"].uniform_(1e-6, 1 - 1e-6)
        m.buf["per"][:nb].copy_(settings_rows(check_settings([None] * nb, nb, V, S)).to(dev))
        lim, flag = min(steps + CHUNK, m._steps), 1                    # (never reached; eos ignored)
        start = m.start[None, :].expand(nb, -1)

        def run(mixed):
            rec = torch.tensor([[ctx[r], lim, flag, 0 if mixed else 1, 0, 0 if mixed else r, 0, 0] for r in range(nb)], dtype=torch.int32)
            m.buf["dialogues"][:nb].copy_(rec)
            if mixed:                                                   # idle slots, armed by the scheduler alone (a 0-step call)
                m.buf["queue"].copy_(torch.tensor([0, nb], dtype=torch.int32))
                m.buf["state"].copy_(m._slot_records([]))
                m._run_steps(1.0, nb, 0, 1.0, True, None, nb, False, True, 0)
            else:
                m.buf["queue"].copy_(torch.tensor([nb, nb], dtype=torch.int32))
                st = m._slot_records(ctx).clone()
                st[:nb, 5], st[:nb, 6] = lim, flag
                m.buf["state"].copy_(st)
                m.buf["x"][:nb].copy_(start)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps // CHUNK):
                m._run_chunk(1.0, nb, 1.0, True, None, nb, False, True, 0 if mixed else None)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e6, m.buf["tokens"][:nb, :, :steps].clone()

        ta, tb = run(False)[1], run(True)[1]
        assert torch.equal(ta, tb), "the mixed entry decodes other tokens than the per-dialogue entry"
        t = {"A": [], "B": []}
        for _ in range(reps):
            t["A"].append(run(False)[0])
            t["B"].append(run(True)[0])
        for k in "AB":
            v = sorted(t[k])
            lines.append(f"  {nb:2d} slots  {k}  min {v[0]:7.1f}  median {med(v):7.1f}  max {v[-1]:7.1f}   all {[round(x, 1) for x in t[k]]}")
        lines.append(f"  {nb:2d} slots  B median - A median = {med(t['B']) - med(t['A']):+.1f} us per step (A's own spread {max(t['A']) - min(t['A']):.1f})")
    # (b)
    n, slots = 96, 64
    kinds = [j % 3 == 0 for j in range(n)]
    lims = torch.randint(100, 609, (n,), generator=g).tolist()
    srcs = [torch.randint(1, 30000, (1, 48), generator=g) for _ in range(n)]
    gi, ui = [j for j in range(n) if kinds[j]], [j for j in range(n) if not kinds[j]]
    sets = [{"cond_scale": 2.0 if k else 1.0} for k in kinds]

    def one_call(lm):
        return m.generate_many(srcs, max_length=608, slots=slots, ignore_eos=True, limits=lm, settings=sets, mixed_guidance=True)

    def two_calls(lm):
        a = m.generate_many([srcs[j] for j in gi], max_length=608, slots=slots, ignore_eos=True, limits=[lm[j] for j in gi], cond_scale=2.0)
        b = m.generate_many([srcs[j] for j in ui], max_length=608, slots=slots, ignore_eos=True, limits=[lm[j] for j in ui])
        return a, b
    one_call([20] * n); two_calls([20] * n)                            # graphs and buffers of the timed shapes
    t = {"one": [], "two": []}
    for _ in range(max(1, min(reps, 3))):
        for name, fn in (("two", two_calls), ("one", one_call)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn(lims)
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)
    useful = sum(lims)
    lines.append(f"(b) {len(gi)} guided (scale 2.0) + {len(ui)} unguided utterances, every third one guided, step limits 100..608 (sum {useful}), eos ignored, "
                 f"{slots} slots, wall time of the call(s) with fresh random draws, encoder included; rounds two one two one ...")
    lines.append(f"  two calls (guided: 32 slot pairs, then unguided: 64 slots)  ms  min {min(t['two']):8.1f}  median {med(t['two']):8.1f}   all {[round(x, 1) for x in t['two']]}")
    lines.append(f"  one mixed call (64 slots, pairs wherever two are idle)      ms  min {min(t['one']):8.1f}  median {med(t['one']):8.1f}   all {[round(x, 1) for x in t['one']]}")
    lines.append(f"  one / two (medians) = {med(t['one']) / med(t['two']):.3f}")
    print("\n".join(lines), flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")


def beam_ab():
    """(a), (b), (c) of BEAM=1 (see the module docstring)"""
    import statistics
    med = statistics.median
    steps, reps, B = int(os.environ.get("STEPS", "256")), int(os.environ.get("REPEATS", "5")), 10
    parts = [p.strip() for p in os.environ.get("PARTS", "a,b,c").split(",")]
    sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(two_output=False, dim=512, dim_target=512), seed=0).items()}
    E = sd["semantic_token_emb.weight"].clone()
    E[-1] = 0.0
    sd["semantic_token_emb.weight"] = E
    m = TextToSemanticDecoder(sd, dev, max_length=2048)
    g = torch.Generator().manual_seed(3)
    srcs = [torch.randint(1, 30000, (1, 48), generator=g) for _ in range(24)]
    lines = [f"text2semantic beam search, full-size CoSingle (synthetic weights, eos row zeroed: no hypothesis finishes), beam size {B}, "
             f"device: {torch.cuda.get_device_name(0)}"]

    def run(n, scale):
        kw = {"cond_scale": scale} if scale > 1.0 else {}
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m.generate_beam(srcs[:n], beam_size=B, max_length=steps, **kw)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        assert all(r["steps"] == steps for r in m.last_beam), "an utterance ended early: the step count is not fixed"
        return dt / steps * 1e6

    sides = [(k, name, n, scale) for k, name, n, scale in (("a", "(a) unguided, 6 utterances = 60 slots", 6, 1.0),
                                                            ("b", "(b) guided 1.5, 3 utterances = 60 slots", 3, 1.5)) if k in parts]
    if sides:
        for _, _, n, scale in sides:                         # graphs and buffers of the timed shapes
            run(n, scale)
        c0 = ops.clock_stamps()
        t = {k: [] for k, _, _, _ in sides}
        for _ in range(reps):
            for k, _, n, scale in sides:
                t[k].append(run(n, scale))
        clk = ops.clock_from_stamps(c0, ops.clock_stamps())
        lines.append(f"us per beam step = wall time of generate_beam / {steps} steps ({steps // CHUNK} graph replays of {CHUNK} steps; encoder, arming and "
                     f"back-track included); {reps} rounds {' '.join(k for k, _, _, _ in sides)} ...; effective shader clock over the timed rounds "
                     f"({clk.get('cus', 0)} CUs): " + (f"{clk['mhz']:.0f} MHz" if clk else "not reported"))
        for k, name, _, _ in sides:
            v = sorted(t[k])
            lines.append(f"  {name:42s} us/step  min {v[0]:8.1f}  median {med(v):8.1f}  max {v[-1]:8.1f}   all {[round(x, 1) for x in t[k]]}")
        if "a" in t and "b" in t:
            lines.append(f"  (b) median / (a) median = {med(t['b']) / med(t['a']):.3f}; per hypothesis-step: (a) {med(t['a']) / 60 * 1e3:.0f} ns at 60 "
                         f"hypotheses, (b) {med(t['b']) / 30 * 1e3:.0f} ns at 30")
    if "c" in parts:
        n, per, scale = 24, 3, 1.5
        lims = torch.randint(100, 609, (n,), generator=g).tolist()
        many = lambda l: m.generate_beam_many(srcs, beam_size=B, max_length=608, limits=l, cond_scale=scale)
        waves = lambda l: [m.generate_beam(srcs[w:w + per], beam_size=B, max_length=max(l[w:w + per]), cond_scale=scale) for w in range(0, n, per)]
        many([20] * n); waves([20] * n)                        # graphs and buffers of the timed shapes
        t = {"many": [], "waves": []}
        c0 = ops.clock_stamps()
        for _ in range(max(1, min(reps, 3))):
            for name, fn in (("waves", waves), ("many", many)):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fn(lims)
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e3)
            assert all(r["steps"] == l for r, l in zip(m.last_beam, lims)), "an utterance ended before its limit"
        clk = ops.clock_from_stamps(c0, ops.clock_stamps())
        lines.append(f"(c) guided (scale {scale}), {n} utterances, step limits 100..608 (sum {sum(lims)}), 60 of 64 slots = 3 groups of 10 slot pairs; wall "
                     f"time, encoder included; rounds waves many ...; effective shader clock: " + (f"{clk['mhz']:.0f} MHz" if clk else "not reported"))
        lines.append(f"  lock-step waves of {per} (each to its longest limit)   ms  min {min(t['waves']):8.1f}  median {med(t['waves']):8.1f}   all {[round(x, 1) for x in t['waves']]}")
        lines.append(f"  generate_beam_many (refilled groups)              ms  min {min(t['many']):8.1f}  median {med(t['many']):8.1f}   all {[round(x, 1) for x in t['many']]}")
        lines.append(f"  many / waves (medians) = {med(t['many']) / med(t['waves']):.3f}")
    print("\n".join(lines), flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")


def rules_ab():
    """D / A / B of RULES=1 (see the module docstring)"""
    import statistics
    from covomix_amd.t2s import check_settings, settings_rows
    med = statistics.median
    steps, warm, reps = int(os.environ.get("STEPS", "256")), int(os.environ.get("WARM", "256")), int(os.environ.get("REPEATS", "5"))
    sides = [x.strip() for x in os.environ.get("SIDES", "D,A,B").split(",")]
    names = {"D": "D default chain", "A": "A per-dialogue chain", "B": "B rules chain (1.3 / 64, 3-gram, min length)"}
    lines = [f"text2semantic history rules, device: {torch.cuda.get_device_name(0)}; sides {' '.join(sides)}; slot b decodes dialogue b, no queue; "
             f"{warm} untimed steps, then {steps} timed = {steps // CHUNK} graph replays of {CHUNK} steps between two synchronisations; "
             f"{reps} rounds {' '.join(sides)} ..."]
    for model, kw in (("CoMix", dict(two_output=True, dim=512, dim_target=1024)), ("CoSingle", dict(two_output=False, dim=512, dim_target=512))):
        sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(**kw), seed=0).items()}
        m = TextToSemanticDecoder(sd, dev, max_length=2048)
        V, S = m.d["vocab"], m.d["streams"]
        g = torch.Generator().manual_seed(3)
        for nb in (8, 64):
            srcs = [torch.randint(1, 30000, (1, 48), generator=g) for _ in range(nb)]
            m._ensure(nb, nb, warm + steps)
            chunk = {"D": lambda: m._run_chunk(1.0, nb), "A": lambda: m._run_chunk(1.0, nb, per=True),
                     "B": lambda: m._run_chunk(1.0, nb, per=True, rules=True)}
            for k in sides:                                  # graphs of the timed shapes (captured on idle slots)
                m._graph(1.0, nb, **({} if k == "D" else {"per": True} if k == "A" else {"per": True, "rules": True}))
            rec = m._slot_records(m._contexts(srcs)).to(dev)
            m.buf["uniforms"].uniform_(1e-6, 1 - 1e-6)
            m.buf["per"][:nb].copy_(settings_rows(check_settings([None] * nb, nb, V, S)).to(dev))
            if "B" in sides:
                from covomix_amd.t2s import check_rules, rules_rows
                m.buf["rules"][:nb].copy_(rules_rows(check_rules(None, nb, m.max_length, 1.3, 64, 3, warm + steps)).to(dev))
            start = m.start[None, :].expand(nb, -1)

            def run(k):
                m.buf["x"][:nb].copy_(start)
                m.buf["state"].copy_(rec)
                for _ in range(warm // CHUNK):
                    chunk[k]()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(steps // CHUNK):
                    chunk[k]()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / steps * 1e6, m.buf["tokens"][:nb, :, :warm + steps].clone()
            tok = {k: run(k)[1] for k in sides}              # warm-up of every timed shape; and what must agree does
            if "D" in tok and "A" in tok:
                assert torch.equal(tok["D"], tok["A"]), "the per-dialogue chain decodes other tokens than the default chain"
            c0 = ops.clock_stamps()
            t = {k: [] for k in sides}
            for _ in range(reps):
                for k in sides:
                    t[k].append(run(k)[0])
            clk = ops.clock_from_stamps(c0, ops.clock_stamps())
            lines.append(f"{model}, {nb} slots; effective shader clock over the timed rounds ({clk.get('cus', 0)} CUs): "
                         + (f"{clk['mhz']:.0f} MHz" if clk else "not reported"))
            for k in sides:
                v = sorted(t[k])
                lines.append(f"  {names[k]:45s} us/step  min {v[0]:8.1f}  median {med(v):8.1f}  max {v[-1]:8.1f}   all {[round(x, 1) for x in t[k]]}")
            if "A" in t and "B" in t:
                rep_ = 0 if "B" not in tok else sum(1 for b in range(nb) for s_ in range(S)
                                                    if len({tuple(tok["B"][b, s_, i:i + 3].tolist()) for i in range(warm + steps - 2)}) < warm + steps - 2)
                lines.append(f"  B median - A median = {med(t['B']) - med(t['A']):+.1f} us per step (A's own spread {max(t['A']) - min(t['A']):.1f}); "
                             f"streams of B with a repeated 3-gram: {rep_} of {nb * S}")
        del m
    print("\n".join(lines), flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "a") as f:
            f.write("\n".join(lines) + "\n")


if os.environ.get("RULES", "0") == "1":
    rules_ab()
    sys.exit(0)
if os.environ.get("PER", "0") == "1":
    per_dialogue_ab()
    sys.exit(0)
if os.environ.get("BEAM", "0") == "1":
    beam_ab()
    sys.exit(0)
if os.environ.get("MIXED", "0") == "1":
    mixed_ab()
    sys.exit(0)
CFG = {"cosingle": dict(two_output=False, dim=512, dim_target=512), "comix": dict(two_output=True, dim=512, dim_target=1024)}
for name in which:
    kw = CFG[name]
    sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(**kw), seed=0).items()}
    m = TextToSemanticDecoder(sd, dev, max_length=2048)
    src = torch.randint(1, 30000, (1, 48))
    wbytes = sum(L[k].numel() * 4 for L in m.dec for k in ("wqkv_s", "wo_s", "wq_c", "wo_c", "w1", "w2")) + m.emb.numel() * 4
    t0 = time.perf_counter(); enc = m.encode(src); torch.cuda.synchronize(); t_enc = time.perf_counter() - t0
    t0 = time.perf_counter(); enc = m.encode(src); torch.cuda.synchronize(); t_enc = time.perf_counter() - t0
    print(f"{name}: encoder {t_enc*1e3:.2f} ms, weights per token step {wbytes/1e6:.1f} MB")
    for nb in BATCHES:                                      # slots decoded together, lock step
        m._ensure(nb, nb, N)
        m._graph(1.0, nb)
        ctx = m._contexts([src] * nb)
        m.buf["uniforms"].uniform_(1e-6, 1 - 1e-6)
        m.buf["x"][:nb].copy_(m.start[None, :].expand(nb, -1))
        m.buf["state"].copy_(m._slot_records(ctx))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(N // CHUNK):
            m._run_chunk(1.0, nb)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        print(f"   batch {nb:2d}: {dt/N*1e6:7.1f} us/step = {nb*N/dt:8.0f} tokens/s; weight streaming {wbytes/(dt/N)/1e12:.2f} TB/s", flush=True)
    if os.environ.get("MANY", "1") == "1":
        # utterances that end at different steps: limits spread over [100, 608]
        g = torch.Generator().manual_seed(3)
        n = int(os.environ.get("UTTS", "64"))
        lims = torch.randint(100, 609, (n,), generator=g).tolist()
        srcs = [torch.randint(1, 30000, (1, 48), generator=g) for _ in range(n)]
        for slots in (8, 32, 64):
            m.generate_many(srcs, max_length=608, slots=slots, ignore_eos=True, limits=[20] * n)      # graph + buffers of the timed shape
            torch.cuda.synchronize(); t0 = time.perf_counter()
            m.generate_many(srcs, max_length=608, slots=slots, ignore_eos=True, limits=lims)
            torch.cuda.synchronize(); t_many = time.perf_counter() - t0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for w in range(0, n, slots):
                m.generate_batch(srcs[w:w + slots], max_length=max(lims[w:w + slots]), ignore_eos=True)
            torch.cuda.synchronize(); t_lock = time.perf_counter() - t0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for w in range(0, n, slots):
                m.generate_batch(srcs[w:w + slots], max_length=608, ignore_eos=True)
            torch.cuda.synchronize(); t_fix = time.perf_counter() - t0
            print(f"   {n} utterances, limits 100..608 (sum {sum(lims)}), {slots} slots: continuous {t_many*1e3:7.1f} ms = {sum(lims)/t_many:8.0f} useful tokens/s;"
                  f" lock step {t_lock*1e3:7.1f} ms = {sum(lims)/t_lock:8.0f}; fixed 608 for all {t_fix*1e3:7.1f} ms = {n*608/t_fix:8.0f} tokens/s", flush=True)
