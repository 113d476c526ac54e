#!/usr/bin/env python3
"""The fixed-grid solvers of the acoustic solve on a full-size SYNTHETIC VoMix (dim 1024, depth 8, 16 heads): what an evaluation costs
under each method and what truncation error it leaves.  A synthetic checkpoint says nothing about audio quality; no default moves.

  time  [--root OTHER] [--rounds 5] [--solves 5]
        ms per solve at the bench shape (B = 8 x T = 1000, cond_scale 0.7).  With --root (another checkout with its library built, the
        parent commit): the default midpoint-32 solve there and here, one fresh process each, alternating, --rounds times - this
        change leaves that path's kernels alone, so its times must lie inside the other checkout's own spread.  Then rk4-32,
        heun3-24 and rk4-16 here, against evaluations x midpoint's time per evaluation.
  error [--frames 1000] [--ref-nfe 512]
        rel-L2 of the final mel of one utterance for every built-in method at 8 ... 64 evaluations, against the named midpoint path
        (the two-call path the parent has) at --ref-nfe evaluations.
  cost  [--solves 5]
        ms per solve at the bench shape with and without the embedded error estimate (return_error) for midpoint-32 and rk4-32: the
        estimate adds one stored stage per step for midpoint, the partial sums and one finishing launch.
  grids [--frames 1000] [--ref-nfe 512]
        rel-L2 of the final mel of one utterance for midpoint, heun3 and rk4 at 16, 24 and 32 evaluations on the uniform grid, sway:-1,
        cosine and the grid fitted from that method's own 64-step error estimate, against midpoint at --ref-nfe evaluations on the
        uniform grid; the fitted grids are printed.  Synthetic weights: where THIS field is hard, nothing about audio quality.

Every timed process is a fresh child of this one (which never touches the GPU), runs under a time limit, and a failure ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(pkg_root):
    sys.path.insert(0, pkg_root)
    import torch
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel
    shapes = syn.acoustic_param_shapes(dim=1024, dim_cond=160, dim_emb=1024, depth=8, heads=16, streams=2)
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed=0).items()}
    sd["transformer.rotary_emb.inv_freq"] = torch.from_numpy(syn.rotary_inv_freq(64))
    return torch, syn, CoVoMixModel.from_state_dict(sd).eval().to("cuda:0")


def worker(pkg_root, settings, solves):
    """one process: [(method, nfe[, estimate])] -> ms per solve (host clock around a solve that ends in a device synchronise), after two
    warm-up solves"""
    torch, syn, model = _model(pkg_root)
    inp = syn.synthetic_inputs("vomix", 8, 1000, 400, seed=3)
    args = [inp["phoneme_ids"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), 0.7]
    y0 = inp["y0"].cuda()
    out = []
    for method, nfe, *flag in settings:
        model.ode_method, model.nfe = method, nfe
        if flag:                             # (a checkout without the estimate is never asked for it)
            model.ode_error = bool(flag[0])
        ms = []
        for i in range(2 + solves):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.synthesis_sample(*args, y0=y0)
            torch.cuda.synchronize()
            if i >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
        out.append(dict(method=method, nfe=nfe, ms=ms, estimate=bool(flag and flag[0])))
    import covomix_amd
    print("RESULT " + json.dumps(dict(package=os.path.dirname(os.path.abspath(covomix_amd.__file__)), runs=out)), flush=True)


def _child(pkg_root, settings, solves):
    cmd = [sys.executable, os.path.abspath(__file__), "_worker", "--root", pkg_root, "--solves", str(solves),
           "--settings", ",".join(":".join(str(x) for x in st) for st in settings)]
    r = subprocess.run(cmd, cwd=pkg_root, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"worker in {pkg_root} failed (exit status {r.returncode}): nothing more is started")
    res = json.loads(lines[-1][7:])
    assert os.path.samefile(os.path.dirname(res["package"]), pkg_root), (res["package"], pkg_root)          # the child imported THAT checkout's package
    return res["runs"]


def _stats(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def study_time(other, rounds, solves):
    print(f"bench shape B = 8 x T = 1000, full-size synthetic VoMix, cond_scale 0.7; {solves} solves per process after 2 warm-up solves")
    here, there = [], []
    if other:
        for r in range(rounds):
            for name, root, acc in (("other", other, there), ("this", ROOT, here)):
                ms = _child(root, [("midpoint", 32)], solves)[0]["ms"]
                acc += ms
                print(f"round {r + 1} {name:5s} midpoint-32: median {_stats(ms)[0]:8.2f} ms  (min {_stats(ms)[1]:.2f}, max {_stats(ms)[2]:.2f})", flush=True)
        for name, acc in (("other checkout", there), ("this checkout", here)):
            med, lo, hi = _stats(acc)
            print(f"{name:15s} midpoint-32 over {rounds} processes: median {med:.2f} ms, min {lo:.2f}, max {hi:.2f}")
        inside = _stats(there)[1] <= _stats(here)[0] <= _stats(there)[2]
        print(f"this checkout's median lies {'inside' if inside else 'OUTSIDE'} the other checkout's spread")
    res = _child(ROOT, [("midpoint", 32), ("rk4", 32), ("heun3", 24), ("rk4", 16)], solves)
    per_eval = _stats(res[0]["ms"])[0] / 32
    print(f"one process, this checkout: midpoint-32 median {_stats(res[0]['ms'])[0]:.2f} ms = {per_eval:.3f} ms per evaluation")
    for r in res[1:]:
        med, lo, hi = _stats(r["ms"])
        print(f"{r['method']:>8s}-{r['nfe']:<3d} median {med:8.2f} ms (min {lo:.2f}, max {hi:.2f}); evaluations x midpoint's time per evaluation "
              f"{per_eval * r['nfe']:8.2f} ms; excess {med - per_eval * r['nfe']:+.2f} ms ({(med / (per_eval * r['nfe']) - 1) * 100:+.2f} %)")


def study_error(frames, ref_nfe):
    os.environ["CVX_GRAPH"] = "0"            # (one solve per setting: capturing each would cost more than it saves)
    torch, syn, model = _model(ROOT)
    from covomix_amd.acoustic import TABLEAUS
    inp = syn.synthetic_inputs("vomix", 1, frames, int(0.4 * frames), seed=3)
    args = [inp["phoneme_ids"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), 0.7]
    y0 = inp["y0"].cuda()

    def solve(method, nfe):
        model.ode_method, model.nfe = method, nfe
        return model.synthesis_sample(*args, y0=y0).double()
    ref = solve("midpoint", ref_nfe)
    print(f"one utterance of {frames} frames, full-size synthetic VoMix (precision {model.precision}), cond_scale 0.7; rel-L2 of the final mel against "
          f"method='midpoint' (the two-call path) at {ref_nfe} evaluations.  Below ~1e-6 the figures are the split-precision kernels' own error.")
    counts = (8, 12, 16, 24, 32, 48, 64)      # (multiples of three: Heun's third-order rule alone, as it has no other)
    print("| evaluations | " + " | ".join(TABLEAUS) + " |")
    print("|---|" + "---|" * len(TABLEAUS))
    for nfe in counts:
        cells = []
        for name, tab in TABLEAUS.items():
            if nfe % tab.stages or (tab.stages == 3) != (nfe % 3 == 0):
                cells.append("-")
                continue
            cells.append(f"{float((solve(name, nfe) - ref).norm() / ref.norm()):.2e}")
        print(f"| {nfe} | " + " | ".join(cells) + " |", flush=True)


def study_cost(solves):
    res = _child(ROOT, [("midpoint", 32, 0), ("midpoint", 32, 1), ("rk4", 32, 0), ("rk4", 32, 1)], solves)
    print(f"bench shape B = 8 x T = 1000, full-size synthetic VoMix, cond_scale 0.7; one process, {solves} solves per setting after 2 warm-up solves")
    for plain, est in (res[0:2], res[2:4]):
        (m0, lo0, hi0), (m1, lo1, hi1) = _stats(plain["ms"]), _stats(est["ms"])
        print(f"{plain['method']:>8s}-{plain['nfe']}: median {m0:.2f} ms (min {lo0:.2f}, max {hi0:.2f}); with the error estimate {m1:.2f} ms "
              f"(min {lo1:.2f}, max {hi1:.2f}): {m1 - m0:+.2f} ms ({(m1 / m0 - 1) * 100:+.2f} %)")


def study_grids(frames, ref_nfe):
    os.environ["CVX_GRAPH"] = "0"
    torch, syn, model = _model(ROOT)
    from covomix_amd.acoustic import TABLEAUS, fit_time_grid
    inp = syn.synthetic_inputs("vomix", 1, frames, int(0.4 * frames), seed=3)
    args = [inp["phoneme_ids"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), 0.7]
    y0 = inp["y0"].cuda()

    def solve(method, nfe, grid="uniform", estimate=False):
        model.ode_method, model.nfe, model.ode_grid, model.ode_error = method, nfe, grid, estimate
        return model.synthesis_sample(*args, y0=y0).double()
    ref = solve("midpoint", ref_nfe)
    print(f"one utterance of {frames} frames, full-size synthetic VoMix (precision {model.precision}), cond_scale 0.7; rel-L2 of the final mel against "
          f"midpoint at {ref_nfe} evaluations on the uniform grid.  'fitted': fit_time_grid on the method's own 64-step uniform estimate.")
    print("| method | evaluations | uniform | sway:-1 | cosine | fitted |")
    print("|---|---|---|---|---|---|")
    fitted = {}
    for name in ("midpoint", "heun3", "rk4"):
        n = TABLEAUS[name].stages
        solve(name, 64 * n, estimate=True)
        err = model.last_solve_error
        print(f"# {name}: delta_rms of the 64-step solve, every 8th step: " + " ".join(f"{float(err.delta_rms[k, 0]):.2e}" for k in range(0, 64, 8)), flush=True)
        for nfe in (16, 24, 32):
            if nfe % n:
                print(f"| {name} | {nfe} | - | - | - | - |")
                continue
            g = fitted[(name, nfe)] = fit_time_grid(err, nfe // n)
            cells = [f"{float((solve(name, nfe, grid) - ref).norm() / ref.norm()):.2e}" for grid in ("uniform", "sway:-1", "cosine", g)]
            print(f"| {name} | {nfe} | " + " | ".join(cells) + " |", flush=True)
    for (name, nfe), g in fitted.items():
        print(f"fitted grid {name}-{nfe}: " + " ".join(f"{t:.4f}" for t in g))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["time", "error", "cost", "grids", "_worker"])
    ap.add_argument("--root", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--settings", default="midpoint:32")
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--ref-nfe", type=int, default=512)
    a = ap.parse_args()
    if a.mode == "_worker":
        worker(a.root or ROOT, [(st[0], *map(int, st[1:])) for st in (s.split(":") for s in a.settings.split(","))], a.solves)
    elif a.mode == "time":
        study_time(a.root and os.path.abspath(a.root), a.rounds, a.solves)
    elif a.mode == "cost":
        study_cost(a.solves)
    elif a.mode == "grids":
        study_grids(a.frames, a.ref_nfe)
    else:
        study_error(a.frames, a.ref_nfe)
