#!/usr/bin/env python3
"""Fit a time grid for the acoustic solve from a measured error table: one fine uniform solve with the method's embedded error estimate
(CoVoMixModel(ode_error=True)), then acoustic.fit_time_grid for the requested number of steps.  Writes the JSON list of grid points that
`--ode_grid FILE` of the generation CLIs reads, and prints the table it was fitted from.

  python tools/fit_time_grid.py --steps 16 --method midpoint --out grid16.json [--acous_ckpt CKPT] [--fine_steps 64]
                                [--batch 4 --frames 500] [--cond_scale 0.7] [--reduce rms]

Without --acous_ckpt the weights are SYNTHETIC (--dim / --depth / --heads: full size by default): such a grid says where this random
field is hard, nothing about a trained checkpoint or about audio quality.  The inputs are synthetic_inputs either way."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def measure(model, inputs, method, steps, cond_scale=0.7, grid="uniform"):
    """acoustic.SolveError of one solve of `steps` steps on the model (its solver settings are put back afterwards)"""
    from covomix_amd.acoustic import resolve_method
    keep = model.nfe, model.ode_method, model.ode_grid, model.ode_error
    try:
        model.nfe, model.ode_method, model.ode_grid, model.ode_error = steps * resolve_method(method).stages, method, grid, True
        model.synthesis_sample(inputs["phoneme_ids"].to(model.device), inputs["cond"].to(model.device), None, cond_scale, y0=inputs["y0"])
        return model.last_solve_error
    finally:
        model.nfe, model.ode_method, model.ode_grid, model.ode_error = keep


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, required=True, help="steps of the fitted grid (nfe / stages of the method)")
    ap.add_argument("--method", default="midpoint")
    ap.add_argument("--out", required=True)
    ap.add_argument("--acous_ckpt", default=None)
    ap.add_argument("--fine_steps", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--prompt_frames", type=int, default=None, help="default: 40 %% of --frames")
    ap.add_argument("--cond_scale", type=float, default=0.7)
    ap.add_argument("--reduce", default="rms", choices=["rms", "mean", "max"])
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--heads", type=int, default=16)
    a = ap.parse_args(argv)
    import torch
    import covomix_amd.synthetic as syn
    from covomix_amd.acoustic import fit_time_grid, resolve_method
    from covomix_amd.conditional_model import CoVoMixModel
    if resolve_method(a.method).b_err is None:
        raise ValueError(f"--method {a.method} has no embedded error estimate")
    if a.acous_ckpt:
        model = CoVoMixModel.load_from_checkpoint(a.acous_ckpt)
    else:
        shapes = syn.acoustic_param_shapes(dim=a.dim, dim_cond=160, dim_emb=a.dim, depth=a.depth, heads=a.heads, streams=2)
        sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed=0).items()}
        sd["transformer.rotary_emb.inv_freq"] = torch.from_numpy(syn.rotary_inv_freq(64))
        model = CoVoMixModel.from_state_dict(sd)
    model = model.eval().to("cuda:0")
    d = model._get_field().d
    kind = "vomix" if d["streams"] == 2 else "vosingle"
    prompt = a.prompt_frames if a.prompt_frames is not None else int(0.4 * a.frames)
    inputs = syn.synthetic_inputs(kind, a.batch, a.frames, prompt, seed=a.seed)
    err = measure(model, inputs, a.method, a.fine_steps, a.cond_scale)
    grid = fit_time_grid(err, a.steps, reduce=a.reduce)
    print(f"{a.method}, {a.fine_steps} uniform steps, {a.batch} x {a.frames} frames, cond_scale {a.cond_scale}: local error of the order-{err.order} "
          f"solution per step ({a.reduce} over the utterances), state RMS")
    for k in range(a.fine_steps):
        print(f"  t = {err.grid[k]:.4f}  delta_rms {float(err.delta_rms[k].square().mean().sqrt()):.3e}  state_rms {float(err.state_rms[k].mean()):.4f}")
    print(f"fitted grid, {a.steps} steps: " + " ".join(f"{t:.5f}" for t in grid))
    with open(a.out, "w") as f:
        json.dump(list(grid), f)
    print("wrote", a.out)
    return grid


if __name__ == "__main__":
    main()
