"""The Runge-Kutta stage kernel (cvx_rk_stage_f32) and the solvers built on it, on the GPU: the kernel against fp64 with a bound
counted from its roundings, its m = 0 form against cvx_cfg_combine_axpy_f32 bit for bit, the generic stage loop against the named
midpoint / Euler path bit for bit, the new methods against the restated integrator (tests/rk_restated.py) driving the CPU oracle,
ragged batches, per-utterance guidance scales and the workspace."""
import ctypes as C

import numpy as np
import pytest
import torch

import rk_restated as rr
from conftest import rel_l2
from test_model_gpu import ROLL_TOL, _state

pytestmark = pytest.mark.gpu

SMALL = dict(dim=128, dim_emb=64, depth=4, heads=2)
GUARD = 64                                 # floats of NaN on either side of every buffer (256 bytes: alignment is kept)
SHAPES = [(1, 1), (1, 3), (3, 85), (1, 255), (1, 256), (1, 257), (131, 80)]


class Guarded:
    """n floats with a NaN band on either side; misalign: the data starts 4 bytes behind a 16-byte boundary"""

    def __init__(self, n, fill=None, misalign=False, gen=None):
        self.buf = torch.full((2 * GUARD + n + 4,), float("nan"), dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo = GUARD + (1 if misalign else 0)
        self.data = self.buf[self.lo:self.lo + n]
        if fill == "randn":
            self.data.copy_(torch.randn(n, generator=gen, dtype=torch.float32))
        elif fill is not None:
            self.data.fill_(fill)
        assert self.data.data_ptr() % 16 == (4 if misalign else 0)

    def bands_untouched(self):
        return bool(self.buf[:self.lo].isnan().all()) and bool(self.buf[self.lo + self.data.numel():].isnan().all())


def _configs():
    """(m, zero pattern over the m + 1 weights, f_n?, scale mode, out aliases y, extra outputs, k_out?, which buffers are misaligned)"""
    n = 0
    for m in range(4):
        for fn_mode in ("none", "scalar", "rows"):
            for mis in ("none", "one", "all"):
                zeros = [(n >> j) & 1 == 1 and (n % 3 != 0) for j in range(m + 1)]       # every third config: no weight is 0
                yield dict(m=m, zeros=zeros, fn=fn_mode != "none", rows_scale=fn_mode == "rows", alias=n % 2 == 0, extra=n % 3,
                           k_out=n % 4 < 2, mis=mis, n=n)
                n += 1


@pytest.mark.parametrize("rows,dim", SHAPES)
def test_stage_kernel_against_fp64(ops, rows, dim):
    """Every element within (m + 3) 2^-24 (|y| + sum |w_j k_j| + |w_m| (|(1 + s) f_c| + |s f_n|)) of the fp64 value of the same fp32
    inputs: one rounding per accumulated stage (m + 1 fused multiply-adds) and the combine's (1 + s, two products, one difference -
    at most the weight of two more on the whole sum).  Counted, not measured.  Guard bands stay NaN, inputs stay as they were."""
    gen = torch.Generator().manual_seed(1000 * rows + dim)
    n = rows * dim
    worst = 0.0
    for cfg in _configs():
        m = cfg["m"]
        names = ["fc", "fn", "y", "k0", "k1", "k2", "k_out", "out", "out2", "out3"]
        mis = {nm: cfg["mis"] == "all" or (cfg["mis"] == "one" and i == cfg["n"] % len(names)) for i, nm in enumerate(names)}
        g = {nm: Guarded(n, "randn", mis[nm], gen) for nm in ("fc", "fn", "y", "k0", "k1", "k2")}
        for nm in ("k_out", "out", "out2", "out3"):
            g[nm] = Guarded(n, None, mis[nm])
        w = [0.0 if z else float(np.float32(torch.randn((), generator=gen).item())) for z in cfg["zeros"]]
        s = float(np.float32(0.7))
        scales = None
        if cfg["rows_scale"]:
            pick = torch.randint(0, 4, (rows,), generator=gen)
            pick[0] = cfg["n"] % 2                                             # (a single row: 1.0 and 0.7 in turn)
            scales = torch.tensor([0.7, 1.0, 2.0, -0.25], dtype=torch.float32)[pick].cuda()
        before = {nm: g[nm].data.clone() for nm in ("fc", "fn", "y", "k0", "k1", "k2")}
        out = g["y"] if cfg["alias"] else g["out"]
        shape = lambda t: t.data.view(rows, dim)
        k_prev = [None if (w[j] == 0.0 and j % 2 == 0) else shape(g[f"k{j}"]) for j in range(m)]     # a stage of weight 0 may be NULL
        ops.rk_stage(shape(g["fc"]), shape(g["fn"]) if cfg["fn"] else None, shape(g["y"]), s, w, shape(out), k_prev=k_prev,
                     k_out=shape(g["k_out"]) if cfg["k_out"] else None, row_scale=scales,
                     out2=shape(g["out2"]) if cfg["extra"] >= 1 else None, out3=shape(g["out3"]) if cfg["extra"] == 2 else None)
        torch.cuda.synchronize()
        # ---- fp64 value and bound
        d = {nm: before[nm].double().view(rows, dim) for nm in before}
        v, vabs = d["fc"], d["fc"].abs()
        if cfg["fn"]:
            sr = scales.double()[:, None] if scales is not None else torch.full((rows, 1), s, dtype=torch.float64, device="cuda")
            comb = d["fc"] * (1 + sr) - sr * d["fn"]
            v = torch.where(sr == 1.0, d["fc"], comb) if scales is not None else comb
            vabs = ((1 + sr) * d["fc"]).abs() + (sr * d["fn"]).abs()
        want, mag = d["y"].clone(), d["y"].abs()
        for j in range(m):
            want += d[f"k{j}"] * w[j]
            mag += (d[f"k{j}"] * w[j]).abs()
        want += v * w[m]
        mag += abs(w[m]) * vabs
        bound = (m + 3) * 2.0 ** -24 * mag
        outs = [out] + [g["out2"]] * (cfg["extra"] >= 1) + [g["out3"]] * (cfg["extra"] == 2)
        for o in outs:
            err = (shape(o).double() - want).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool((err <= bound).all()), (cfg, ratio)
        assert torch.equal(shape(outs[0]), shape(outs[-1]))
        if cfg["k_out"]:
            kerr = (shape(g["k_out"]).double() - v).abs()
            assert bool((kerr <= 3 * 2.0 ** -24 * vabs).all()), cfg
            if scales is not None:
                at_one = scales == 1.0
                assert torch.equal(shape(g["k_out"])[at_one], before["fc"].view(rows, dim)[at_one])
        # ---- nothing else was written
        for nm in names:
            assert g[nm].bands_untouched(), (nm, cfg)
        for nm in before:
            if not (nm == "y" and cfg["alias"]):
                assert torch.equal(g[nm].data, before[nm]), (nm, cfg)
        for nm, used in (("k_out", cfg["k_out"]), ("out", not cfg["alias"]), ("out2", cfg["extra"] >= 1), ("out3", cfg["extra"] == 2)):
            if not used:
                assert bool(g[nm].data.isnan().all()), (nm, cfg)
    print(f"FIGURE rk_stage {rows}x{dim}: largest error / bound {worst:.3f}")


@pytest.fixture
def ops():
    from covomix_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("rows,dim,misalign", [(131, 80, False), (3, 85, False), (1, 257, True), (1, 1, False), (64, 80, True)])
def test_without_stored_stages_the_bits_are_cfg_combine_axpy(ops, rows, dim, misalign):
    gen = torch.Generator().manual_seed(rows + dim)
    n = rows * dim
    fc, fn, y = (Guarded(n, "randn", misalign, gen).data.view(rows, dim) for _ in range(3))
    for f_n in (fn, None):
        for s, coef in ((0.7, 0.0625), (0.7, 0.03125), (2.0, -0.3), (1.0, 0.125), (0.0, 1.0)):
            a = [torch.empty_like(y) for _ in range(3)]
            b = [Guarded(n, None, misalign).data.view(rows, dim) for _ in range(3)]
            ops.cfg_combine_axpy(fc, f_n, y, s, coef, *a)
            ops.rk_stage(fc, f_n, y, s, [coef], b[0], out2=b[1], out3=b[2])
            for x, z in zip(a, b):
                assert torch.equal(x, z), (s, coef, f_n is None)
    ya, yb = y.clone(), y.clone()                                          # in place
    ops.cfg_combine_axpy(fc, fn, ya, 0.7, 0.5, ya)
    ops.rk_stage(fc, fn, yb, 0.7, [0.5], yb)
    assert torch.equal(ya, yb) and not torch.equal(ya, y)


def test_rows_at_scale_one_take_the_conditional_branch(ops):
    rows, dim = 37, 80
    gen = torch.Generator().manual_seed(5)
    fc, fn, y = (torch.randn(rows, dim, generator=gen).cuda() for _ in range(3))
    scales = torch.full((rows,), 0.7)
    scales[::3] = 1.0
    scales = scales.cuda()
    k, out = torch.empty_like(y), torch.empty_like(y)
    ops.rk_stage(fc, fn, y, 123.0, [0.25], out, k_out=k, row_scale=scales)       # (the scalar is not used beside row scales)
    one = scales == 1.0
    assert torch.equal(k[one], fc[one])
    ref = torch.empty_like(y)
    ops.cfg_combine_axpy(fc, fn, torch.zeros_like(y), 0.7, 1.0, ref)
    assert torch.equal(k[~one], ref[~one])                                      # the other rows: the scalar kernel's combine at 0.7
    assert not torch.equal(k[one], ref[one])
    # a SCALAR scale of 1.0 with a null branch given is the formula (2 f_c - f_n): the caller decides not to pass f_n
    ops.rk_stage(fc, fn, y, 1.0, [0.25], out, k_out=k)
    assert torch.equal(k, fc * 2.0 - fn)


def test_refusals_launch_nothing(ops):
    from covomix_amd import _lib
    lib = _lib.load()
    rows, dim = 5, 16
    t = lambda: torch.full((rows, dim), 7.0, device="cuda")
    fc, fn, y, k0, scale = t(), t(), t(), t(), torch.full((rows,), 0.7, device="cuda")
    k_out, out, out2, out3 = t(), t(), t(), t()

    def call(f_c=fc, f_n=fn, y_=y, row_scale=None, k_prev=(k0,), w=(0.5, 0.5), m=1, out_=out, rows_=rows, dim_=dim):
        kp = (C.c_void_p * 4)(*[None if k is None else k.data_ptr() for k in k_prev])
        wa = (C.c_float * 5)(*w)
        p = lambda x: None if x is None else x.data_ptr()
        return lib.cvx_rk_stage_f32(p(f_c), p(f_n), p(y_), 0.7, p(row_scale), kp, wa, m, k_out.data_ptr(), p(out_), out2.data_ptr(),
                                    out3.data_ptr(), rows_, dim_, ops._stream())
    bad = [dict(f_c=None), dict(y_=None), dict(out_=None), dict(m=4, k_prev=(k0,) * 4, w=(0.1,) * 5), dict(m=-1),
           dict(k_prev=(None,)), dict(m=2, k_prev=(k0, None), w=(0.5, 0.5, 0.5)), dict(rows_=-1), dict(dim_=0), dict(dim_=-3),
           dict(f_n=None, row_scale=scale)]
    for kw in bad:
        assert call(**kw) == -22, kw
        assert lib.cvx_last_error_string()
    torch.cuda.synchronize()
    for o in (k_out, out, out2, out3, y):
        assert bool((o == 7.0).all())
    assert call(k_prev=(None,), w=(0.0, 0.5)) == 0 and call(rows_=0) == 0       # a NULL stage of weight 0 and an empty batch are fine
    torch.cuda.synchronize()
    assert bool((out != 7.0).all()) and torch.equal(out, out2) and torch.equal(out, out3)


# ------------------------------------------------------------------------------------------------ the solvers
@pytest.fixture(scope="module")
def small():
    from covomix_amd.conditional_model import CoVoMixModel
    sd = _state("vomix", **SMALL)
    return sd, CoVoMixModel.from_state_dict(sd, nfe=8).eval().to("cuda:0")


@pytest.fixture(scope="module")
def inputs():
    import covomix_amd.synthetic as syn
    return syn.synthetic_inputs("vomix", 3, 131, 40, seed=99)


def _oracle(sd, ids, cond, y0, scale, name, nfe):
    """the restated integrator on the CPU oracle's field, fp32"""
    import covomix_oracle as orc
    a, b, c = rr.as_floats(name)
    assert nfe % len(b) == 0
    grid = torch.from_numpy(rr.grid_f32(nfe // len(b)))
    fn = lambda t, x: orc.forward_with_cond_scale(sd, x, t, ids, cond, scale)
    return rr.odeint_rk(fn, y0, grid, a, b, c)


def _run(model, inp, scale, method, nfe, sl=slice(None)):
    model.ode_method, model.nfe = method, nfe
    return model.synthesis_sample(inp["phoneme_ids"][sl].cuda(), inp["cond"][sl].cuda(), None, scale, y0=inp["y0"][sl])


@pytest.mark.parametrize("graph", ["0", "1"])
def test_explicit_tableau_has_the_bits_of_the_named_path(small, graph, monkeypatch):
    """method='midpoint' / 'euler' run the two-call path on cvx_cfg_combine_axpy_f32, the same tableau given explicitly runs the generic
    stage loop on cvx_rk_stage_f32: equal bits, eager and through the captured graph, call after call."""
    import covomix_amd.synthetic as syn
    from covomix_amd.acoustic import TABLEAUS
    monkeypatch.setenv("CVX_GRAPH", graph)
    sd, model = small
    inp = syn.synthetic_inputs("vomix", 2, 50, 15, seed=3)
    for name, nfe in (("midpoint", 8), ("euler", 6)):
        named = _run(model, inp, 0.7, name, nfe)
        first, second = _run(model, inp, 0.7, TABLEAUS[name], nfe), _run(model, inp, 0.7, TABLEAUS[name], nfe)
        assert torch.equal(first, named) and torch.equal(second, named), name
        assert torch.equal(_run(model, inp, 0.7, name, nfe), named)
        assert bool(named.isfinite().all()) and not torch.equal(named.cpu(), inp["y0"])


@pytest.mark.parametrize("name,nfe", [("heun2", 8), ("rk4", 8), ("rk4_classic", 8), ("heun3", 9)])
def test_new_methods_against_the_oracle(small, inputs, name, nfe):
    """Against the restated integrator driving the oracle's CFG-combined field in fp32, at the rollout tolerance of the project.  At
    these sizes the methods differ from one another by 1e-2 and more: a wrong tableau or a fall-through to Euler is far outside."""
    sd, model = small
    out = _run(model, inputs, 0.7, name, nfe)
    ref = _oracle(sd, inputs["phoneme_ids"], inputs["cond"], inputs["y0"], 0.7, name, nfe)
    e = rel_l2(out, ref)
    print(f"FIGURE {name} nfe {nfe}: rel-L2 against the oracle {e:.3e}")
    assert e < ROLL_TOL


def test_new_methods_on_vosingle_and_in_fp32(inputs):
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel
    sd1 = _state("vosingle", **SMALL)
    m1 = CoVoMixModel.from_state_dict(sd1, nfe=8, ode_method="rk4").eval().to("cuda:0")
    one = syn.synthetic_inputs("vosingle", 1, 77, 20, seed=4)
    e1 = rel_l2(_run(m1, one, 0.7, "rk4", 8), _oracle(sd1, one["phoneme_ids"], one["cond"], one["y0"], 0.7, "rk4", 8))
    sd = _state("vomix", **SMALL)
    m32 = CoVoMixModel.from_state_dict(sd, nfe=9, ode_method="heun3", precision="fp32").eval().to("cuda:0")
    sl = slice(0, 1)
    e2 = rel_l2(_run(m32, inputs, 0.7, "heun3", 9, sl),
                _oracle(sd, inputs["phoneme_ids"][sl], inputs["cond"][sl], inputs["y0"][sl], 0.7, "heun3", 9))
    print(f"FIGURE vosingle rk4 {e1:.3e}, fp32 heun3 {e2:.3e}")
    assert e1 < ROLL_TOL and e2 < ROLL_TOL


LENGTHS = (131, 37, 1)


def _ragged(model, inp, scale, method, nfe):
    model.ode_method, model.nfe = method, nfe
    cut = lambda k: [inp[k][i, :L].cuda() for i, L in enumerate(LENGTHS)]
    return model.synthesis_sample(cut("phoneme_ids"), cut("cond"), None, scale, y0=cut("y0"))


def _single(model, inp, i, L, scale, method, nfe):
    model.ode_method, model.nfe = method, nfe
    return model.synthesis_sample(inp["phoneme_ids"][i:i + 1, :L].cuda(), inp["cond"][i:i + 1, :L].cuda(), None, scale,
                                  y0=inp["y0"][i:i + 1, :L])[0]


def test_ragged_batch_equals_single_calls(small, inputs):
    sd, model = small
    outs = _ragged(model, inputs, 0.7, "rk4", 8)
    for i, L in enumerate(LENGTHS):
        assert tuple(outs[i].shape) == (L, 80)
        e = rel_l2(outs[i], _single(model, inputs, i, L, 0.7, "rk4", 8))
        print(f"FIGURE ragged rk4 utterance {i} ({L} frames): rel-L2 against its own call {e:.3e}")
        assert e < 1e-5


SCALES = (1.0, 0.7, 2.0)


@pytest.mark.parametrize("method,nfe", [("midpoint", 8), ("rk4", 8)])
def test_per_utterance_scales(small, method, nfe):
    """One scale per utterance in one batch: every utterance within 1e-5 of its own scalar call and within ROLL_TOL of the oracle at
    its scale (midpoint: oracle.sample; rk4: the restated integrator on the oracle's field).  Equal values are the scalar path; other
    values replay the same graph."""
    import covomix_amd.synthetic as syn
    import covomix_oracle as orc
    sd, model = small
    f = model._get_field()
    inp = syn.synthetic_inputs("vomix", 3, 50, 15, seed=7)
    out = _run(model, inp, list(SCALES), method, nfe)
    graphs = f.__dict__.get("_graphs", {})
    n_graphs = len(graphs)
    assert sum("per-row" in k and method in k for k in graphs) == 1
    other = (2.0, 1.0, 0.5)
    out_b = _run(model, inp, torch.tensor(other), method, nfe)
    graphs = f.__dict__.get("_graphs", {})
    assert len(graphs) == n_graphs and sum("per-row" in k and method in k for k in graphs) == 1     # the second mix replayed the first one's graph
    same = _run(model, inp, [0.7, 0.7, 0.7], method, nfe)
    assert torch.equal(same, _run(model, inp, 0.7, method, nfe))
    for i in range(3):
        sl = slice(i, i + 1)
        for res, scales in ((out, SCALES), (out_b, other)):
            e = rel_l2(res[sl], _run(model, inp, scales[i], method, nfe, sl))
            assert e < 1e-5, (method, i, scales[i], e)
        if method == "midpoint":
            ref = orc.sample(sd, inp["phoneme_ids"][sl], inp["cond"][sl], inp["y0"][sl], SCALES[i], nfe=nfe)
        else:
            ref = _oracle(sd, inp["phoneme_ids"][sl], inp["cond"][sl], inp["y0"][sl], SCALES[i], method, nfe)
        e = rel_l2(out[sl], ref)
        print(f"FIGURE per-utterance scale {SCALES[i]} {method}: rel-L2 against the oracle {e:.3e}")
        assert e < ROLL_TOL
    with pytest.raises(ValueError):
        _run(model, inp, [0.7, 1.0], method, nfe)


@pytest.mark.parametrize("method,nfe", [("midpoint", 8), ("rk4", 8)])
def test_per_utterance_scales_in_a_ragged_batch(small, inputs, method, nfe):
    import covomix_oracle as orc
    sd, model = small
    outs = _ragged(model, inputs, list(SCALES), method, nfe)
    for i, L in enumerate(LENGTHS):
        e = rel_l2(outs[i], _single(model, inputs, i, L, SCALES[i], method, nfe))
        assert e < 1e-5, (method, i, e)
        ids, cond, y0 = (inputs[k][i:i + 1, :L] for k in ("phoneme_ids", "cond", "y0"))
        ref = orc.sample(sd, ids, cond, y0, SCALES[i], nfe=nfe) if method == "midpoint" else _oracle(sd, ids, cond, y0, SCALES[i], method, nfe)
        e = rel_l2(outs[i], ref[0])
        print(f"FIGURE ragged per-utterance scale {SCALES[i]} {method} ({L} frames): rel-L2 against the oracle {e:.3e}")
        assert e < ROLL_TOL
    same = _ragged(model, inputs, [0.7] * 3, method, nfe)
    for x, z in zip(same, _ragged(model, inputs, 0.7, method, nfe)):
        assert torch.equal(x, z)


def test_stage_buffers_exist_from_first_use_only():
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel
    model = CoVoMixModel.from_state_dict(_state("vomix", **SMALL), nfe=8).eval().to("cuda:0")
    f = model._get_field()
    inp = syn.synthetic_inputs("vomix", 2, 50, 15, seed=3)
    _run(model, inp, 0.7, "midpoint", 8)
    _run(model, inp, 1.0, "euler", 6)
    model.ode_method, model.nfe = "midpoint", 8
    model.synthesis_sample([inp["phoneme_ids"][0, :20].cuda()], [inp["cond"][0, :20].cuda()], None, 0.7, y0=[inp["y0"][0, :20]])
    assert len(f._ws) == 3 and all("rk_k" not in ws for ws in f._ws.values())
    _run(model, inp, 0.7, "heun3", 9)
    ws = f._ws[(4, 50)]
    assert [tuple(k.shape) for k in ws["rk_k"]] == [(100, 80)]                       # Heun's third-order rule reads one stored stage
    _run(model, inp, 0.7, "rk4", 8)
    assert [tuple(k.shape) for k in ws["rk_k"]] == [(100, 80)] * 3                   # at most three: rows x dim_out floats each
    assert all("rk_k" not in w for key, w in f._ws.items() if key != (4, 50))
