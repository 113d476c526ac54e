"""Non-uniform time grids, embedded pairs and the grid fitter of the acoustic solve, host side (no GPU): evaluation times against the
numpy restatements bit for bit, every refusal, the lower-order weights against the order conditions in exact fractions, the fitter on
an analytic problem with a sharp feature, and the ABI and code objects of the two new kernels."""
import math
import os
import re
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

import grid_restated as gr
import rk_restated as rr
from conftest import ROOT
from covomix_amd.acoustic import (TABLEAUS, FlowMatchingSampler, SolveError, Tableau, evaluation_times, fit_time_grid, resolve_grid,
                                  time_grid)

NAMES = ("euler", "midpoint", "heun2", "heun3", "rk4", "rk4_classic")
PAIRS = ("midpoint", "heun2", "heun3", "rk4", "rk4_classic")


# ------------------------------------------------------------------------------------------------ times
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("steps", [1, 2, 16])
def test_default_and_explicit_uniform_grid_have_the_restated_bits(name, steps):
    n = TABLEAUS[name].stages
    want_t, want_dt = rr.evaluation_times(steps, name)
    uniform = time_grid("uniform", steps)
    assert list(uniform) == [float(x) for x in rr.grid_f32(steps)]
    for grid in (None, "uniform", uniform, list(uniform), np.asarray(uniform)):
        times, dts = evaluation_times(steps * n, name, grid)
        assert times.dtype == torch.float32 and times.tolist() == want_t and dts == want_dt, (name, steps, type(grid))
    assert resolve_grid(uniform, steps * n, name) is None and resolve_grid("uniform", steps * n, name) is None     # today's keys


@pytest.mark.parametrize("spec", ["uniform", "cosine", "sway:-1", "sway:-0.5", "sway:0", "sway:1", f"sway:{gr.SWAY_MAX!r}"])
@pytest.mark.parametrize("steps", [1, 2, 7, 16, 64])
def test_named_grids(spec, steps):
    g = time_grid(spec, steps)
    assert isinstance(g, tuple) and len(g) == steps + 1 and all(isinstance(x, float) for x in g)
    assert g[0] == 0.0 and g[-1] == 1.0 and all(a < b for a, b in zip(g[:-1], g[1:]))
    assert all(float(np.float32(x)) == x for x in g)                       # fp32 holds every point exactly
    assert list(g) == [float(x) for x in gr.named_grid(spec, steps)], spec
    hash(g)


def test_sway_takes_small_steps_first_and_cosine_at_both_ends():
    h = np.diff(time_grid("sway:-1", 16))
    assert all(a < b for a, b in zip(h[:-1], h[1:]))
    h = np.diff(time_grid("cosine", 16))
    assert h[0] < h[7] and h[-1] < h[8] and abs(h[0] - h[-1]) < 1e-6


@pytest.mark.parametrize("name", PAIRS + ("euler",))
@pytest.mark.parametrize("spec", ["sway:-1", "cosine"])
def test_times_on_a_named_grid_equal_the_restatement_bit_for_bit(name, spec):
    n = TABLEAUS[name].stages
    want_t, want_dt = gr.evaluation_times(gr.named_grid(spec, 8), name)
    times, dts = evaluation_times(8 * n, name, spec)
    assert times.tolist() == want_t and dts == want_dt
    times2, dts2 = evaluation_times(8 * n, name, time_grid(spec, 8))
    assert times2.tolist() == want_t and dts2 == want_dt
    assert abs(sum(dts) - 1.0) < 1e-6 and len(set(dts)) > 1


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("grid,word", [
    ([0.0, 0.5, 1.0], "points"),                                           # wrong length (3 steps asked)
    ([0.0, 0.25, 0.5, 0.75, 1.0], "points"),
    ([0.0, 0.5, 0.5, 1.0], "entry 2"),                                     # not strictly increasing
    ([0.0, 0.6, 0.4, 1.0], "entry 2"),
    ([0.0, 0.5, 0.50000001, 1.0], "entry 2"),                              # increasing in fp64, equal in fp32
    ([0.1, 0.4, 0.7, 1.0], "entry 0"),                                     # ends
    ([0.0, 0.4, 0.7, 0.9], "entry 3"),
    ([0.0, 0.4, 0.7, 1.0000001], "entry 3"),
    ([0.0, float("nan"), 0.7, 1.0], "entry 1"),                            # non-finite
    ([0.0, 0.4, float("inf"), 1.0], "entry 2"),
    ([0.0, 1e-45, 0.5, 1.0], "entry 1"),                                   # midpoint's stage time rounds onto t0
    ("sway:-1.01", "sway"), ("sway:1.76", "sway"), ("sway:nan", "sway"), ("sway:x", "sway"), ("sway:", "sway"),
    ("linear", "linear"), ("", "unknown"), (5, "neither"), ([0.0, "a", 0.5, 1.0], "neither"),
])
def test_a_bad_grid_is_refused_by_name(grid, word):
    for call in (lambda: evaluation_times(6, "midpoint", grid), lambda: resolve_grid(grid, 6, "midpoint"),
                 lambda: FlowMatchingSampler(None, 6, "midpoint", grid=grid)):
        with pytest.raises(ValueError) as e:
            call()
        assert word in str(e.value), str(e.value)


def test_a_step_too_small_for_a_stage_is_refused_per_method():
    tiny = float(np.float32(2.0 ** -149))                                  # the smallest step fp32 has: t0 + dt / 2 is t0 or t1
    grid = [0.0, tiny, 0.5, 1.0]
    time_grid(grid, 3)                                                     # a grid as such
    evaluation_times(3, "euler", grid)                                     # no stage strictly inside a step
    evaluation_times(6, "heun2", grid)
    for name in ("midpoint", "heun3", "rk4", "rk4_classic"):
        with pytest.raises(ValueError):
            evaluation_times(3 * TABLEAUS[name].stages, name, grid)
    near_one = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    with pytest.raises(ValueError) as e:
        evaluation_times(6, "midpoint", [0.0, 0.5, near_one, 1.0])
    assert "entry 3" in str(e.value)
    with pytest.raises(ValueError):
        evaluation_times(7, "midpoint", "cosine")                          # nfe is still checked first


# ------------------------------------------------------------------------------------------------ embedded pairs
@pytest.mark.parametrize("name", PAIRS)
def test_lower_order_weights_in_exact_arithmetic(name):
    """sum b_err = 1; order 2 where the table says so: b_err . c = 1/2 - and not order 3 (b_err . c^2 != 1/3); order 1 otherwise
    (b_err . c != 1/2).  The package's floats are these fractions."""
    a, b, c, order = rr.TABLEAUS[name]
    be, q = gr.B_ERR[name]
    dot = lambda u, v: sum((x * y for x, y in zip(u, v)), Fr(0))
    assert len(be) == len(b) and sum(be, Fr(0)) == 1 and tuple(be) != tuple(b)
    assert q < order
    if q == 2:
        assert dot(be, c) == Fr(1, 2) and dot(be, [x * x for x in c]) != Fr(1, 3)
    else:
        assert q == 1 and dot(be, c) != Fr(1, 2)
    t = TABLEAUS[name]
    assert t.b_err == tuple(float(x) for x in be) and t.err_order == q


def test_tableau_validates_b_err():
    assert TABLEAUS["euler"].b_err is None and TABLEAUS["euler"].err_order is None
    mid = ((0.5,),), (0.0, 1.0), (0.0, 0.5)
    assert Tableau("m", *mid).b_err is None                                # existing constructions stay valid
    t = Tableau("m", *mid, [1, 0])
    assert t.b_err == (1.0, 0.0) and t.err_order == 1 and t == Tableau("m", *mid) and hash(t) == hash(Tableau("m", *mid))
    assert Tableau("m", *mid, b_err=(0.5, 0.5)).err_order == 1
    for bad in ((1.0,), (1.0, 0.0, 0.0), (0.5, 0.4), (float("nan"), 1.0), (float("inf"), 0.0), (0.0, 1.0), ("x", 1.0), 1.0):
        with pytest.raises(ValueError):
            Tableau("m", *mid, bad)
    with pytest.raises(ValueError):                                        # return_error needs a pair
        FlowMatchingSampler(None, 4, "euler")._error_state([3], True)
    with pytest.raises(ValueError):
        FlowMatchingSampler(None, 4, Tableau("m", *mid))._error_state([3], True)
    assert FlowMatchingSampler(None, 4, "euler")._error_state([3], False) is None


# ------------------------------------------------------------------------------------------------ the fitter
def _sharp_error(name, steps=64):
    """SolveError of a uniform fp64 solve of the sharp problem with the restated integrator"""
    a, b, c = rr.as_floats(name)
    be, q = gr.B_ERR[name]
    grid = time_grid("uniform", steps)
    y0 = torch.tensor([1.0, 0.0], dtype=torch.float64)
    _, deltas, states = gr.odeint_rk_err(gr.sharp_field, y0, torch.tensor(grid, dtype=torch.float64), a, b, c, tuple(float(x) for x in be))
    rms = lambda xs: torch.stack([x.square().mean().sqrt() for x in xs])[:, None]
    return SolveError(grid=grid, method=name, order=q, delta_rms=rms(deltas), state_rms=rms(states))


@pytest.fixture(scope="module")
def sharp_errors():
    return {name: _sharp_error(name) for name in ("midpoint", "heun2", "heun3", "rk4")}


@pytest.mark.parametrize("steps", [8, 16, 32])
@pytest.mark.parametrize("name", ["midpoint", "heun2", "heun3", "rk4"])
def test_fitted_grid_halves_the_global_error_on_a_sharp_problem(name, steps, sharp_errors):
    """y' = w(t) (-y2, y1) with a bump of w at t = 0.85 (closed form through erf).  The grid fitted from the 64-step estimate has at
    most half the uniform grid's global error (measured in fp64: ratios from 5.2 - heun2, 8 steps - to 226 - heun3, 16 steps)."""
    a, b, c = rr.as_floats(name)
    y0, exact = torch.tensor([1.0, 0.0], dtype=torch.float64), gr.sharp_exact()
    fitted = fit_time_grid(sharp_errors[name], steps)
    err = lambda g: float((rr.odeint_rk(gr.sharp_field, y0, torch.tensor(g, dtype=torch.float64), a, b, c) - exact).norm())
    e_u, e_f = err(time_grid("uniform", steps)), err(fitted)
    print(f"FIGURE {name} {steps} steps: uniform {e_u:.3e}, fitted {e_f:.3e}, ratio {e_u / e_f:.1f}")
    assert e_f <= 0.5 * e_u
    h = np.diff(fitted)
    assert h[np.searchsorted(fitted, 0.85) - 1] < 1.0 / steps < h[0]       # small steps on the bump, large ones before it


@pytest.mark.parametrize("name", ["midpoint", "rk4"])
def test_fitter_agrees_with_its_numpy_restatement(name, sharp_errors):
    e = sharp_errors[name]
    for steps in (8, 24):
        got = fit_time_grid(e, steps)
        want = gr.fit(e.delta_rms[:, 0].numpy(), e.grid, e.order, steps)
        assert len(got) == steps + 1 and got[0] == 0.0 and got[-1] == 1.0 and all(x < y for x, y in zip(got[:-1], got[1:]))
        assert np.abs(np.asarray(got) - want.astype(np.float64)).max() <= 2.0 ** -23       # one fp32 spacing below 1


def test_equal_errors_give_the_uniform_grid_and_the_reductions():
    for name, old, new in (("midpoint", 64, 16), ("rk4", 64, 64), ("heun3", 16, 8), ("midpoint", 10, 10), ("heun2", 7, 7)):
        e = SolveError(grid=time_grid("uniform", old), method=name, order=TABLEAUS[name].err_order,
                       delta_rms=torch.full((old, 3), 1e-3, dtype=torch.float64), state_rms=torch.ones(old, 3, dtype=torch.float64))
        for reduce in ("rms", "mean", "max"):
            assert fit_time_grid(e, new, reduce=reduce) == time_grid("uniform", new), (name, old, new, reduce)
    # the reductions differ when the utterances do: one utterance with all its error in the last quarter
    d = torch.full((16, 2), 1e-3, dtype=torch.float64)
    d[12:, 1] = 1.0
    e = SolveError(grid=time_grid("uniform", 16), method="midpoint", order=1, delta_rms=d, state_rms=torch.ones(16, 2, dtype=torch.float64))
    g_max, g_mean = fit_time_grid(e, 16, "max"), fit_time_grid(e, 16, "mean")
    assert g_max != g_mean and sum(t > 0.75 for t in g_max) > 4
    with pytest.raises(ValueError):
        fit_time_grid(e, 16, "median")
    with pytest.raises(ValueError):
        fit_time_grid(SolveError(e.grid, "midpoint", 1, d[:5], d[:5]), 16)
    with pytest.raises(ValueError):
        fit_time_grid(SolveError(e.grid, "midpoint", 1, d * float("nan"), d), 16)


# ------------------------------------------------------------------------------------------------ model, CLI (nothing runs)
def test_model_and_cli_validate_the_grid_before_anything_runs(tmp_path):
    import json
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel
    from covomix_amd.generation import build_parser, ode_grid_argument, run
    shapes = syn.acoustic_param_shapes(dim=128, dim_cond=160, dim_emb=64, depth=2, heads=2, streams=2)
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes).items()}
    m = CoVoMixModel.from_state_dict(sd)
    assert m.ode_grid == "uniform" and m.ode_error is False and m.last_solve_error is None
    m = CoVoMixModel.from_state_dict(sd, ode_method="rk4", nfe=8, ode_grid="sway:-1", ode_error=True)
    assert m.ode_grid == "sway:-1" and m.ode_error is True
    for kw in (dict(ode_grid="sway:9"), dict(ode_grid=[0.0, 1.0]), dict(ode_grid="nope")):
        with pytest.raises(ValueError):
            CoVoMixModel.from_state_dict(sd, **kw)
    args = build_parser().parse_args([])
    assert args.ode_grid == "uniform" and args.ode_error_json is None
    path = tmp_path / "grid.json"
    path.write_text(json.dumps(list(time_grid("cosine", 16))))
    assert ode_grid_argument(str(path)) == time_grid("cosine", 16) and ode_grid_argument("sway:-1") == "sway:-1"
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps(list(time_grid("cosine", 8))))
    for argv in (["--ode_grid", "sway:5"], ["--ode_grid", str(tmp_path / "none.json")], ["--ode_grid", str(bad)],
                 ["--ode_method", "euler", "--ode_error_json", str(tmp_path / "e.json")]):
        with pytest.raises(ValueError):
            run(False, argv)


# ------------------------------------------------------------------------------------------------ ABI, code objects
def test_abi_of_the_error_estimate_kernels():
    from covomix_amd import _lib, ops
    lib = _lib.load()
    assert lib.cvx_version() == 113
    hdr = open(os.path.join(ROOT, "include", "covomix_hip.h")).read()
    assert re.search(r"#define\s+CVX_ABI_VERSION\s+113\b", hdr)
    rows = int(re.search(r"#define\s+CVX_RK_ERR_ROWS\s+(\d+)", hdr).group(1))
    assert rows == ops.RK_ERR_ROWS and rows >= 1
    for name in ("cvx_rk_stage_err_f32", "cvx_rk_err_finish_f32"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_error_estimate_code_objects_use_no_scratch():
    """The two instances of the last-stage kernel (16-byte and 4-byte accesses) and the finisher in the built library: no private
    segment; the stage kernel's LDS is the eight floats of its block reduction."""
    from covomix_amd import _lib
    from test_attention_form_d import _gfx950_kernel_descriptors
    kds = {k: v for k, v in _gfx950_kernel_descriptors(_lib.LIB_PATH).items() if "rk_err_" in k}
    assert len(kds) == 3 and sum("rk_err_stage_kernel" in k for k in kds) == 2 and sum("rk_err_finish_kernel" in k for k in kds) == 1, sorted(kds)
    for name, (group, private, vgprs) in kds.items():
        print(f"FIGURE {name}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
        assert private == 0 and group == (32 if "stage" in name else 0), (name, group, private)
