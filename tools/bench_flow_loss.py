#!/usr/bin/env python3
"""Dev: what the flow-matching loss costs (CoVoMixModel.flow_matching_loss, csrc/flow_loss.hip).

  python tools/bench_flow_loss.py [--kinds vomix,vosingle] [--precisions f16x3,fp32]
      On the full-size synthetic VoMix / VoSingle, for the batches 8 x 1000 frames and 16 utterances of 400 .. 1200 frames:
        * one flow_matching_loss call (wall time, everything from host tensors to the host result) and the device time of its
          evaluation alone (cfm_inputs + evaluate_seq_times + masked_mse on resident inputs, device events);
        * the yardstick: one field evaluation of the same row count in the existing solve on the non-deferred split route
          (VectorField.prepare + evaluate at one time for all rows, CVX_DEFER_NORM=0 - stand-alone norms, no per-time weight copies);
        * the three new kernels alone against the bytes they move.
      ROUNDS (10) timed rounds after WARM (2); median (min .. max) and the effective shader clock beside every figure.
One JSON line per figure; OUT=file appends them there.  Random-weight models: the figures say nothing about quality."""
import argparse
import json
import os
import statistics
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="vomix,vosingle")
    ap.add_argument("--precisions", default="f16x3,fp32")
    args = ap.parse_args()
    os.environ["CVX_DEFER_NORM"] = "0"          # the yardstick's route; an evaluation with a time per sequence never defers
    rounds, warm = int(os.environ.get("ROUNDS", "10")), int(os.environ.get("WARM", "2"))
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import covomix_amd.synthetic as syn
    import flow_loss_restated as rs
    from covomix_amd import ops
    from covomix_amd.conditional_model import CoVoMixModel
    assert torch.cuda.is_available(), "bench_flow_loss.py measures on the GPU"
    dev = torch.device("cuda:0")

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

    def clocked(fn):
        c0 = ops.clock_stamps()
        t = fn()
        clk = ops.clock_from_stamps(c0, ops.clock_stamps())
        return t, (round(clk["mhz"]) if clk else None)

    g = torch.Generator().manual_seed(0)
    batches = {"8x1000": [1000] * 8, "16x400..1200": [int(x) for x in torch.randint(400, 1201, (16,), generator=g)]}
    for kind in args.kinds.split(","):
        two = kind == "vomix"
        shapes = syn.acoustic_param_shapes(dim_cond=160 if two else 80, streams=2 if two else 1)
        sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed=0).items()}
        sd["transformer.rotary_emb.inv_freq"] = torch.from_numpy(syn.rotary_inv_freq(64))
        for precision in args.precisions.split(","):
            model = CoVoMixModel.from_state_dict(sd, precision=precision).eval().to(dev)
            field = model._get_field()
            for name, lengths in batches.items():
                utts = [rs.utterance(kind, T, seed=T + i) for i, T in enumerate(lengths)]
                M, n = sum(lengths), len(lengths)
                times = [float(x) for x in torch.rand(n, generator=g)]
                call = lambda: model.flow_matching_loss([u["phoneme_ids"] for u in utts], [u["mel"] for u in utts], cond_mels=[u["cond"] for u in utts],
                                                        masks=[u["mask"] for u in utts], times=times, x0=[u["x0"] for u in utts], max_rows=1 << 20)

                def wall():
                    t = []
                    for r in range(warm + rounds):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        res = call()
                        if r >= warm:
                            t.append((time.perf_counter() - t0) * 1e3)
                    return t, res
                (t_wall, res), clk_w = clocked(wall)
                # the evaluation alone, inputs resident
                cat = lambda k, dt=None: torch.cat([u[k] for u in utts]).to(dev) if dt is None else torch.cat([u[k] for u in utts]).to(dev, dt)
                x1, x0, cond, mask, ids = cat("mel"), cat("x0"), cat("cond"), cat("mask", torch.uint8), cat("phoneme_ids")
                t_d, rg = torch.tensor(times, device=dev), ops.Ragged(lengths, dev)
                flow, cond_in = torch.empty_like(x1), torch.empty_like(cond)

                def loss_eval():
                    w = field.xin_rows(lengths)
                    ops.cfm_inputs(x1, x0, cond, mask, t_d, rg, 0.0, w, flow, cond_in)
                    pred = field.evaluate_seq_times(ids, cond_in, w, t_d, lengths)
                    return ops.masked_mse(pred, flow, mask, rg)
                t_eval, clk_e = clocked(lambda: events(loss_eval))
                # the yardstick: one evaluation of the existing solve at one time for all rows (prepare + evaluate; stand-alone norms)
                one_t = torch.tensor([0.31], device=dev)

                def solve_eval():
                    ctx = field.prepare(ids, cond, one_t, False, lengths=lengths)
                    ctx["ws"]["xin"].copy_(x0)
                    field.evaluate(ctx, 0)
                t_ref, clk_r = clocked(lambda: events(solve_eval))
                # the three kernels alone
                pred = field.evaluate_seq_times(ids, cond_in, field.xin_rows(lengths), t_d, lengths)
                h, normed = torch.randn(M, field.d["dim"], device=dev), torch.empty(M, field.d["dim"], device=dev)
                table = torch.randn(n, field.d["depth"], 4, field.d["dim"], device=dev)
                w = field.xin_rows(lengths)
                t_in, clk_i = clocked(lambda: events(lambda: ops.cfm_inputs(x1, x0, cond, mask, t_d, rg, 0.0, w, flow, cond_in)))
                t_mse, _ = clocked(lambda: events(lambda: ops.masked_mse(pred, flow, mask, rg)))
                t_norm, _ = clocked(lambda: events(lambda: ops.adarmsnorm_seq(h, table[:, 0, 0], table[:, 0, 1], normed, rg)))
                t_norm1, _ = clocked(lambda: events(lambda: ops.adarmsnorm(h, table[0, 0, 0], table[0, 0, 1], normed)))
                C, D = cond.shape[1], field.d["dim"]
                gbs = lambda nbytes, t: round(nbytes / statistics.median(t) / 1e6, 1)
                say({"what": "flow loss", "device": torch.cuda.get_device_name(0), "kind": kind, "precision": precision, "batch": name, "rows": M,
                     "loss": round(res.loss, 6), "call_wall_ms": med(t_wall), "clock_mhz_wall": clk_w,
                     "inputs_evaluation_mse_device_ms": med(t_eval), "clock_mhz": clk_e,
                     "solve_evaluation_same_rows_device_ms": med(t_ref), "clock_mhz_solve": clk_r,
                     "ratio_to_solve_evaluation": round(statistics.median(t_eval) / statistics.median(t_ref), 3),
                     "cfm_inputs_ms": med(t_in), "cfm_inputs_gb_s": gbs(M * 4 * (4 * 80 + 2 * C), t_in), "clock_mhz_kernels": clk_i,
                     "masked_mse_two_launches_ms": med(t_mse), "masked_mse_gb_s": gbs(M * 4 * (2 * 80 + 2), t_mse),
                     "adarmsnorm_seq_ms": med(t_norm), "adarmsnorm_seq_gb_s": gbs(M * D * 8, t_norm),
                     "adarmsnorm_one_row_ms": med(t_norm1), "adarmsnorm_one_row_gb_s": gbs(M * D * 8, t_norm1)})
            del model, field
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
