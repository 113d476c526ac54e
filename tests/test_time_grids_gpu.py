"""The embedded error estimate (cvx_rk_stage_err_f32, cvx_rk_err_finish_f32) and the non-uniform time grids on the GPU: the kernel
against fp64 with a counted bound and against cvx_rk_stage_f32 bit for bit, the invariance of a sequence's sums under its place in
the batch, the refusals, and the solves built on them against the restated integrator driving the CPU oracle."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import grid_restated as gr
import rk_restated as rr
from conftest import rel_l2
from test_model_gpu import ROLL_TOL
from test_ode_solvers_gpu import GUARD, LENGTHS, Guarded, _ragged, _run, _single, inputs, small      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture
def ops():
    from covomix_amd import ops as _ops
    return _ops


def _R():
    from covomix_amd import ops as _ops
    return _ops.RK_ERR_ROWS


def _length_sets():
    R = _R()
    return [[1], [R - 1], [R], [R + 1], [2 * R + 3, 1, R]]


def test_block_map_cuts_every_sequence_from_its_own_first_row(ops):
    R = ops.RK_ERR_ROWS
    m = ops.RkErrMap([2 * R + 3, 1, R], "cuda")
    want = [(0, R, 0), (R, R, 0), (2 * R, 3, 0), (2 * R + 3, 1, 1), (2 * R + 4, R, 2)]
    assert m.host.dtype == torch.int32 and m.host.tolist() == [list(w) for w in want] and m.dev.cpu().tolist() == m.host.tolist()
    assert (m.rows, m.n_seq, m.blocks) == (3 * R + 4, 3, 5)
    with pytest.raises(ValueError):
        ops.RkErrMap([3, 0], "cuda")


def _configs():
    """m, zero patterns over w and we, f_n mode, out aliases y, extra outputs, misaligned buffer: 24 configurations that cover m = 0..3
    with every f_n mode, zeros in either weight array (both at once included: such a stage may be NULL) and a we that is all zero"""
    n = 0
    for m in range(4):
        for fn_mode in ("none", "scalar", "rows"):
            for variant in range(2):
                zw = [(n >> j) & 1 == 1 and variant == 1 for j in range(m + 1)]
                ze = [((n + 1) >> (m - j)) & 1 == 1 and (n % 3 != 0) for j in range(m + 1)]
                if n == 13:
                    ze = [True] * (m + 1)
                yield dict(m=m, zw=zw, ze=ze, fn=fn_mode != "none", rows_scale=fn_mode == "rows", alias=n % 2 == 0, extra=n % 3, n=n)
                n += 1


def _depth(cnt, V, chunks):
    """roundings on the longest path of a sequence's sum: the fused multiply-adds of one thread (every 256 V-th group of V elements of
    the chunk), six butterfly levels, three additions over the waves, one addition per chunk in the finisher"""
    per_thread = -(-cnt // (256 * V)) * V
    return per_thread + 6 + 3 + chunks


@pytest.mark.parametrize("dim,misalign", [(80, False), (3, False), (80, True)])
@pytest.mark.parametrize("lengths", _length_sets(), ids=lambda l: "-".join(map(str, l)))
def test_error_stage_kernel_against_fp64_and_the_stage_kernel(ops, lengths, dim, misalign):
    """out, out2, out3 and k_out bit-equal to cvx_rk_stage_f32 on the same arguments.  The two sums of every sequence against fp64 on the same
    fp32 inputs.  Per element delta and o carry at most (m + 3) u (sum of the magnitudes of their terms), u = 2^-24: one rounding per
    fused multiply-add and the combine's three (test_ode_solvers_gpu.test_stage_kernel_against_fp64).  A sum of squares S = sum x_i^2
    computed from x_i + e_i through D roundings on its longest path differs from S by at most
        sum (2 |x_i| e_i + e_i^2) + 1.01 (D + 1) u sum (|x_i| + e_i)^2 ,
    D = _depth(...) counted from the kernel's geometry (dim 80 aligned: 16-byte form, V = 4; otherwise V = 1).  Counted, not measured.
    Every buffer sits between NaN bands; step 1 of a two-step partials buffer is written, step 0 stays NaN."""
    R = ops.RK_ERR_ROWS
    rows, B = sum(lengths), len(lengths)
    n = rows * dim
    gen = torch.Generator().manual_seed(1000 * rows + dim + int(misalign))
    emap = ops.RkErrMap(lengths, "cuda")
    V = 4 if (dim % 4 == 0 and not misalign) else 1
    worst = 0.0
    for cfg in _configs():
        m = cfg["m"]
        names = ["fc", "fn", "y", "k0", "k1", "k2", "out", "out2", "out3", "kout", "ref", "ref2", "ref3", "kref"]
        mis = {nm: misalign and i == cfg["n"] % 10 for i, nm in enumerate(names)}
        g = {nm: Guarded(n, "randn", mis[nm], gen) for nm in ("fc", "fn", "y", "k0", "k1", "k2")}
        for nm in names[6:]:
            g[nm] = Guarded(n, None, mis[nm])
        keep_k = cfg["n"] % 4 < 2
        partials, sums = Guarded(2 * emap.blocks * 2), Guarded(B * 2)
        w = [0.0 if z else float(np.float32(torch.randn((), generator=gen).item())) for z in cfg["zw"]]
        we = [0.0 if z else float(np.float32(torch.randn((), generator=gen).item())) for z in cfg["ze"]]
        s = float(np.float32(0.7))
        scales = None
        if cfg["rows_scale"]:
            pick = torch.randint(0, 4, (rows,), generator=gen)
            pick[0] = 1                                                        # a row at exactly 1.0
            scales = torch.tensor([0.7, 1.0, 2.0, -0.25], dtype=torch.float32)[pick].cuda()
        before = {nm: g[nm].data.clone() for nm in ("fc", "fn", "y", "k0", "k1", "k2")}
        shape = lambda t: t.data.view(rows, dim)
        k_prev = [None if (w[j] == 0.0 and we[j] == 0.0 and j % 2 == 0) else shape(g[f"k{j}"]) for j in range(m)]
        common = dict(row_scale=scales, k_prev=k_prev)
        fn = shape(g["fn"]) if cfg["fn"] else None
        # the plain stage kernel first (it must not see y after an aliased update)
        ops.rk_stage(shape(g["fc"]), fn, shape(g["y"]), s, w, shape(g["ref"]), k_out=shape(g["kref"]) if keep_k else None,
                     out2=shape(g["ref2"]) if cfg["extra"] >= 1 else None, out3=shape(g["ref3"]) if cfg["extra"] == 2 else None, **common)
        out = g["y"] if cfg["alias"] else g["out"]
        pview = partials.data.view(2, emap.blocks, 2)
        ops.rk_stage_err(shape(g["fc"]), fn, shape(g["y"]), s, w, we, shape(out), emap, pview[1], k_out=shape(g["kout"]) if keep_k else None,
                         out2=shape(g["out2"]) if cfg["extra"] >= 1 else None, out3=shape(g["out3"]) if cfg["extra"] == 2 else None, **common)
        ops.rk_err_finish(pview[1:], emap, sums.data.view(1, B, 2))
        torch.cuda.synchronize()
        # ---- the stage kernel's bits
        assert torch.equal(out.data, g["ref"].data), cfg
        if cfg["extra"] >= 1:
            assert torch.equal(g["out2"].data, g["ref2"].data), cfg
        if cfg["extra"] == 2:
            assert torch.equal(g["out3"].data, g["ref3"].data), cfg
        if keep_k:
            assert torch.equal(g["kout"].data, g["kref"].data), cfg
        # ---- fp64 values and bounds
        d = {nm: before[nm].double().view(rows, dim) for nm in before}
        v, vabs = d["fc"], d["fc"].abs()
        if cfg["fn"]:
            sr = scales.double()[:, None] if scales is not None else torch.full((rows, 1), s, dtype=torch.float64, device="cuda")
            comb = d["fc"] * (1 + sr) - sr * d["fn"]
            v = torch.where(sr == 1.0, d["fc"], comb) if scales is not None else comb
            vabs = ((1 + sr) * d["fc"]).abs() + (sr * d["fn"]).abs()
        o, omag = d["y"].clone(), d["y"].abs()
        delta, dmag = torch.zeros_like(o), torch.zeros_like(o)
        for j in range(m):
            o += d[f"k{j}"] * w[j]
            omag += (d[f"k{j}"] * w[j]).abs()
            delta += d[f"k{j}"] * we[j]
            dmag += (d[f"k{j}"] * we[j]).abs()
        o += v * w[m]
        omag += abs(w[m]) * vabs
        delta += v * we[m]
        dmag += abs(we[m]) * vabs
        got = sums.data.view(B, 2).double()
        r0 = 0
        for q, L in enumerate(lengths):
            sl = slice(r0, r0 + L)
            r0 += L
            D = max(_depth(min(L, R) * dim, v_, -(-L // R)) for v_ in ((V,) if not misalign else (1, 4)))   # (the misaligned buffer may be one this configuration does not use)
            for col, (x, mag) in enumerate(((delta, dmag), (o, omag))):
                xs, es = x[sl].abs(), (m + 3) * U * mag[sl]
                want = float(x[sl].square().sum())
                bound = float((2 * xs * es + es * es).sum() + 1.01 * (D + 1) * U * (xs + es).square().sum())
                e = abs(float(got[q, col]) - want)
                worst = max(worst, e / max(bound, 1e-300))
                assert e <= bound, (cfg, q, col, float(got[q, col]), want, bound)
            if all(x == 0.0 for x in we):
                assert float(got[q, 0]) == 0.0
        # ---- nothing else was written
        for nm in names:
            assert g[nm].bands_untouched(), (nm, cfg)
        assert partials.bands_untouched() and sums.bands_untouched() and bool(pview[0].isnan().all())
        for nm in before:
            if not (nm == "y" and cfg["alias"]):
                assert torch.equal(g[nm].data, before[nm]), (nm, cfg)
        for nm, used in (("out", not cfg["alias"]), ("out2", cfg["extra"] >= 1), ("out3", cfg["extra"] == 2), ("kout", keep_k)):
            if not used:
                assert bool(g[nm].data.isnan().all()), (nm, cfg)
    print(f"FIGURE rk_stage_err {lengths} x {dim}{' misaligned' if misalign else ''}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("dim", [80, 3])
def test_a_sequences_sums_do_not_depend_on_its_neighbours(ops, dim):
    """One sequence of 2 R + 3 rows alone, first, last and in the middle of a packed batch, and twice in a row: the same bits."""
    R = ops.RK_ERR_ROWS
    L = 2 * R + 3
    gen = torch.Generator().manual_seed(dim)
    own = [torch.randn(L, dim, generator=gen) for _ in range(5)]                # fc, fn, y, k0, k1
    scale_own = torch.tensor([0.7, 1.0, 2.0])[torch.randint(0, 3, (L,), generator=gen)]
    w, we = [0.25, 0.0, 0.5], [0.125, -0.375, 0.0625]

    def sums_of(lengths, at):
        rows = sum(lengths)
        r0 = sum(lengths[:at])
        bufs = [torch.randn(rows, dim, generator=gen) for _ in range(5)]
        scale = torch.full((rows,), 0.3)
        for b, o_ in zip(bufs, own):
            b[r0:r0 + L] = o_
        scale[r0:r0 + L] = scale_own
        fc, fn, y, k0, k1 = (b.cuda() for b in bufs)
        emap = ops.RkErrMap(lengths, "cuda")
        partials = torch.zeros(1, emap.blocks, 2, device="cuda")
        sums = torch.zeros(1, len(lengths), 2, device="cuda")
        out = torch.empty_like(y)
        ops.rk_stage_err(fc, fn, y, 0.0, w, we, out, emap, partials[0], k_prev=[k0, k1], row_scale=scale.cuda())
        ops.rk_err_finish(partials, emap, sums)
        return sums[0, at].cpu(), out[r0:r0 + L].cpu()
    alone, out_alone = sums_of([L], 0)
    assert float(alone[0]) > 0 and float(alone[1]) > 0
    for lengths, at in (([L], 0), ([L, 5, R], 0), ([R + 1, 7, L], 2), ([1, L, 2 * R], 1), ([R - 1, L], 1)):
        got, out = sums_of(lengths, at)
        assert torch.equal(got, alone) and torch.equal(out, out_alone), (lengths, at, got.tolist(), alone.tolist())


def test_refusals_launch_nothing(ops):
    from covomix_amd import _lib
    lib = _lib.load()
    R = ops.RK_ERR_ROWS
    rows, dim = R + 5, 16
    t = lambda: torch.full((rows, dim), 7.0, device="cuda")
    fc, fn, y, k0, scale = t(), t(), t(), t(), torch.full((rows,), 0.7, device="cuda")
    k_out, out, out2, out3 = t(), t(), t(), t()
    emap = ops.RkErrMap([rows], "cuda")
    partials = torch.full((emap.blocks, 2), 7.0, device="cuda")
    sums = torch.full((1, 1, 2), 7.0, device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def call(f_c=fc, f_n=fn, y_=y, row_scale=None, k_prev=(k0,), w=(0.5, 0.5), we=(0.5, -0.5), m=1, out_=out, rows_=rows, dim_=dim,
             map_dev=emap.dev, map_host=emap.host, blocks=emap.blocks, part=partials):
        kp = (C.c_void_p * 4)(*[None if k is None else k.data_ptr() for k in k_prev])
        wa = (C.c_float * 5)(*w)
        wea = None if we is None else (C.c_float * 5)(*we)
        return lib.cvx_rk_stage_err_f32(p(f_c), p(f_n), p(y_), 0.7, p(row_scale), kp, wa, wea, m, k_out.data_ptr(), p(out_), out2.data_ptr(),
                                        out3.data_ptr(), rows_, dim_, p(map_dev), p(map_host), blocks, p(part), ops._stream())
    i32 = lambda rows_: torch.tensor(rows_, dtype=torch.int32).reshape(-1, 3)
    bad_maps = [i32([(0, R, 0)]),                                 # covers R of R + 5 rows
                i32([(0, R, 0), (R, 6, 0)]),                      # one row too many
                i32([(0, R, 0), (R + 1, 4, 0)]),                  # a gap
                i32([(0, R + 5, 0)]),                             # a chunk above CVX_RK_ERR_ROWS
                i32([(0, 5, 0), (5, R, 0)]),                      # a short chunk that does not end its sequence
                i32([(0, R, 1), (R, 5, 0)]),                      # sequences out of order
                i32([(0, R, 0), (R, 0, 0), (R, 5, 0)]),           # an empty chunk
                i32([(0, R, -1), (R, 5, 0)])]
    bad = [dict(f_c=None), dict(y_=None), dict(out_=None), dict(m=4, k_prev=(k0,) * 4, w=(0.1,) * 5, we=(0.1,) * 5), dict(m=-1),
           dict(k_prev=(None,)), dict(k_prev=(None,), w=(0.0, 0.5)), dict(rows_=-1), dict(dim_=0), dict(f_n=None, row_scale=scale),
           dict(we=None), dict(map_dev=None), dict(map_host=None), dict(part=None), dict(blocks=-1), dict(rows_=rows - 1), dict(rows_=rows + 1),
           dict(blocks=1)] + [dict(map_host=mh, blocks=mh.shape[0]) for mh in bad_maps]
    for kw in bad:
        assert call(**kw) == -22, kw
        assert lib.cvx_last_error_string()
    fin = lambda part=partials, mp=emap.dev, blocks=emap.blocks, steps=1, n_seq=1, err=sums: lib.cvx_rk_err_finish_f32(
        p(part), p(mp), blocks, steps, n_seq, p(err), ops._stream())
    for kw in (dict(part=None), dict(mp=None), dict(err=None), dict(blocks=-1), dict(steps=-1), dict(n_seq=-1)):
        assert fin(**kw) == -22, kw
    torch.cuda.synchronize()
    for o in (k_out, out, out2, out3, y, partials, sums):
        assert bool((o == 7.0).all())
    assert call(k_prev=(None,), w=(0.0, 0.5), we=(0.0, 0.5)) == 0 and fin() == 0 and fin(steps=0) == 0       # a NULL stage of weight 0 twice is fine
    torch.cuda.synchronize()
    assert bool((out != 7.0).all()) and torch.equal(out, out2) and bool((partials != 7.0).all()) and bool((sums != 7.0).all())


# ------------------------------------------------------------------------------------------------ the solves
PAIRS = [("midpoint", 8), ("heun2", 8), ("heun3", 9), ("rk4", 8), ("rk4_classic", 8)]
# The CPU oracle's own fp32-against-fp64 distance in delta_rms on these inputs (3 x 131 frames, seed 99, cond_scale 0.7), the restated
# integrator driving it in either precision; largest relative difference over steps and utterances: midpoint 3.25e-7, heun2 1.69e-7,
# heun3 4.09e-7, rk4 1.87e-7, rk4_classic 3.75e-7.  The bound is four times the largest of them (a maximum over twelve roundings-driven
# entries is itself noisy from method to method; one figure for the set).
ORACLE_DELTA_DISTANCE = 4.094e-7
DELTA_TOL = 4 * ORACLE_DELTA_DISTANCE


def _model_error(model, inp, scale, method, nfe, grid="uniform", sl=slice(None)):
    model.ode_grid, model.ode_error = grid, True
    try:
        y = _run(model, inp, scale, method, nfe, sl)
        return y, model.last_solve_error
    finally:
        model.ode_grid, model.ode_error = "uniform", False


def _oracle_tables(sd, inp, scale, name, grid):
    """(y, delta_rms, state_rms) of the restated integrator on the CPU oracle's field in fp32, on an fp32 grid"""
    import covomix_oracle as orc
    a, b, c = rr.as_floats(name)
    be = tuple(float(x) for x in gr.B_ERR[name][0])
    fn = lambda t, x: orc.forward_with_cond_scale(sd, x, t, inp["phoneme_ids"], inp["cond"], scale)
    y, ds, ys = gr.odeint_rk_err(fn, inp["y0"], torch.from_numpy(np.asarray(grid, dtype=np.float32)), a, b, c, be)
    rms = lambda xs: torch.stack([x.double().square().mean(dim=(1, 2)).sqrt() for x in xs])
    return y, rms(ds), rms(ys)


@pytest.fixture(scope="module")
def oracle_tables(small, inputs):
    sd, _ = small
    return {name: _oracle_tables(sd, inputs, 0.7, name, rr.grid_f32(nfe // len(rr.TABLEAUS[name][1]))) for name, nfe in PAIRS}


@pytest.mark.parametrize("graph", ["0", "1"])
@pytest.mark.parametrize("name,nfe", PAIRS)
def test_error_estimate_end_to_end(small, inputs, oracle_tables, name, nfe, graph, monkeypatch):
    """y with the estimate is y without it, bit for bit (midpoint: the generic stage loop against the named two-call path), eager and
    replayed.  delta_rms within DELTA_TOL = 4 x 4.094e-7 = 1.64e-6 (relative, every step and utterance) of the restated integrator
    driving the oracle in fp32 - four times the oracle's own fp32-against-fp64 distance on these inputs, see ORACLE_DELTA_DISTANCE;
    state_rms within ROLL_TOL: |rms(y) - rms(ref)| <= rms(y - ref), the rollout's own measure."""
    from covomix_amd.acoustic import SolveError, time_grid
    monkeypatch.setenv("CVX_GRAPH", graph)
    sd, model = small
    plain = _run(model, inputs, 0.7, name, nfe)
    y, err = _model_error(model, inputs, 0.7, name, nfe)
    y2, err2 = _model_error(model, inputs, 0.7, name, nfe)
    assert torch.equal(y, plain) and torch.equal(y2, plain) and torch.equal(_run(model, inputs, 0.7, name, nfe), plain)
    steps = nfe // len(rr.TABLEAUS[name][1])
    assert isinstance(err, SolveError) and err.grid == time_grid("uniform", steps) and err.method == name and err.order == gr.B_ERR[name][1]
    assert tuple(err.delta_rms.shape) == tuple(err.state_rms.shape) == (steps, 3) and err.delta_rms.device.type == "cpu"
    assert torch.equal(err.delta_rms, err2.delta_rms) and torch.equal(err.state_rms, err2.state_rms)          # run to run
    _, d_ref, s_ref = oracle_tables[name]
    e_d = float(((err.delta_rms - d_ref).abs() / d_ref).max())
    e_s = float(((err.state_rms - s_ref).abs() / s_ref).max())
    print(f"FIGURE {name} nfe {nfe} graph {graph}: delta_rms {float(d_ref.min()):.3e} .. {float(d_ref.max()):.3e}, largest relative difference "
          f"to the oracle {e_d:.3e} (bound {DELTA_TOL:.3e}); state_rms {e_s:.3e} (bound {ROLL_TOL:.0e})")
    assert e_d <= DELTA_TOL and e_s <= ROLL_TOL


def test_eager_and_replayed_tables_are_the_same_bits(small, inputs, monkeypatch):
    sd, model = small
    got = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("CVX_GRAPH", graph)
        got[graph] = _model_error(model, inputs, 0.7, "rk4", 8)
    assert torch.equal(got["0"][0], got["1"][0])
    assert torch.equal(got["0"][1].delta_rms, got["1"][1].delta_rms) and torch.equal(got["0"][1].state_rms, got["1"][1].state_rms)


def test_methods_without_a_pair_are_refused(small, inputs):
    from covomix_amd.acoustic import TABLEAUS, Tableau
    sd, model = small
    t = TABLEAUS["heun2"]
    for method, nfe in (("euler", 6), (Tableau("heun2_plain", t.a, t.b, t.c), 8)):
        with pytest.raises(ValueError):
            _model_error(model, inputs, 0.7, method, nfe)
    y, err = _model_error(model, inputs, 0.7, Tableau("heun2_pair", t.a, t.b, t.c, (1.0, 0.0)), 8)           # an explicit pair runs
    assert err.order == 1 and torch.equal(y, _run(model, inputs, 0.7, "heun2", 8))


@pytest.mark.parametrize("name,nfe", [("midpoint", 8), ("rk4", 8)])
def test_non_uniform_grids_against_the_oracle(small, inputs, name, nfe, monkeypatch):
    """sway:-1 and a grid fitted from the solve's own estimate: against the restated integrator on the same grid driving the oracle,
    inside ROLL_TOL.  Two grids of equal length share neither graph nor tables: different results, each its eager run's bits."""
    from covomix_amd.acoustic import fit_time_grid, time_grid
    sd, model = small
    steps = nfe // len(rr.TABLEAUS[name][1])
    _, err = _model_error(model, inputs, 0.7, name, nfe)
    fitted = fit_time_grid(err, steps)
    assert len(fitted) == steps + 1 and fitted != time_grid("uniform", steps)
    outs = {}
    for label, grid in (("sway:-1", "sway:-1"), ("fitted", fitted)):
        model.ode_grid = grid
        try:
            monkeypatch.setenv("CVX_GRAPH", "1")
            first, again = _run(model, inputs, 0.7, name, nfe), _run(model, inputs, 0.7, name, nfe)
            monkeypatch.setenv("CVX_GRAPH", "0")
            eager = _run(model, inputs, 0.7, name, nfe)
        finally:
            model.ode_grid = "uniform"
        assert torch.equal(first, eager) and torch.equal(again, eager), label
        assert sum(time_grid(grid, steps) in k for k in model._get_field().__dict__.get("_graphs", {})) == 1, label    # its own graph
        ref, _, _ = _oracle_tables(sd, inputs, 0.7, name, time_grid(grid, steps))
        e = rel_l2(eager, ref)
        print(f"FIGURE {name} nfe {nfe} on {label} {[round(t, 4) for t in time_grid(grid, steps)]}: rel-L2 against the oracle {e:.3e}")
        assert e < ROLL_TOL
        outs[label] = eager
    monkeypatch.setenv("CVX_GRAPH", "1")
    uniform = _run(model, inputs, 0.7, name, nfe)
    assert not torch.equal(outs["sway:-1"], outs["fitted"]) and not torch.equal(outs["sway:-1"], uniform) and not torch.equal(outs["fitted"], uniform)
    keys = model._get_field().__dict__.get("_graphs", {})
    model.ode_grid = time_grid("uniform", steps)                               # the uniform points given explicitly: the uniform solve's graph and bits
    try:
        n_graphs = len(keys)
        assert torch.equal(_run(model, inputs, 0.7, name, nfe), uniform) and len(model._get_field().__dict__["_graphs"]) == n_graphs
    finally:
        model.ode_grid = "uniform"


def test_ragged_batch_error_rows_equal_single_calls(small, inputs):
    """Every utterance's error columns within 1e-5 (relative, per entry) of its own B = 1 call - the tolerance the ragged test has for y:
    the field itself differs by summation order there."""
    sd, model = small
    model.ode_error = True
    try:
        outs = _ragged(model, inputs, 0.7, "rk4", 8)
        err = model.last_solve_error
        assert tuple(err.delta_rms.shape) == (2, len(LENGTHS))
        model.ode_error = False
        plain = _ragged(model, inputs, 0.7, "rk4", 8)
        model.ode_error = True
        for i, L in enumerate(LENGTHS):
            assert torch.equal(outs[i], plain[i])
            y1 = _single(model, inputs, i, L, 0.7, "rk4", 8)
            e1 = model.last_solve_error
            assert rel_l2(outs[i], y1) < 1e-5
            for got, want in ((err.delta_rms[:, i], e1.delta_rms[:, 0]), (err.state_rms[:, i], e1.state_rms[:, 0])):
                e = float(((got - want).abs() / want).max())
                print(f"FIGURE ragged utterance {i} ({L} frames): largest relative difference to its own call {e:.3e}")
                assert e < 1e-5
    finally:
        model.ode_error = False


def test_cli_reads_a_fitted_grid_and_writes_the_error_tables(tmp_path):
    import importlib.util
    from conftest import ROOT
    from covomix_amd import generation
    from covomix_amd.acoustic import time_grid
    from test_generation_gpu import _write_fixture
    tmp = str(tmp_path)
    _write_fixture(tmp, "vomix")
    spec = importlib.util.spec_from_file_location("fit_time_grid_tool", os.path.join(ROOT, "tools", "fit_time_grid.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    gpath = os.path.join(tmp, "grid.json")
    grid = tool.main(["--steps", "4", "--method", "midpoint", "--fine_steps", "8", "--batch", "2", "--frames", "50", "--out", gpath,
                      "--acous_ckpt", os.path.join(tmp, "acous.ckpt")])
    assert json.load(open(gpath)) == list(grid) and len(grid) == 5 and grid[0] == 0.0 and grid[-1] == 1.0
    tdir, pdir = os.path.join(tmp, "text"), os.path.join(tmp, "prompt")
    os.makedirs(tdir); os.makedirs(pdir)
    g = np.random.RandomState(0)
    for n, k in (("utt_a", 60), ("utt_b", 37)):
        for suf in ("_1", "_2"):
            np.save(os.path.join(pdir, f"{n}{suf}.hubert_code.npy"), g.randint(0, 510, size=30))
            np.save(os.path.join(pdir, f"{n}{suf}.mel.npy"), (g.randn(80, 30) * 2 - 6).astype(np.float32))
        np.save(os.path.join(tdir, f"{n}.semantic.npy"), g.randint(0, 510, size=(2, k)))
    base = ["--acous_ckpt", os.path.join(tmp, "acous.ckpt"), "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"), "--text_dir", tdir,
            "--prompt_dir", pdir, "--mode", "covomix", "--seed", "30", "--nfe", "8", "--ode_grid", gpath]
    epath = os.path.join(tmp, "err.json")
    assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, "a"), "--ode_error_json", epath]) == 2
    assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, "b")]) == 2
    assert generation.run(True, base[:-2] + ["--saved_dir", os.path.join(tmp, "c")]) == 2
    tables = json.load(open(epath))
    assert sorted(tables) == ["utt_a", "utt_b"]
    for n in tables:
        (seg,) = tables[n]
        assert seg["grid"] == list(grid) and seg["method"] == "midpoint" and seg["order"] == 1
        assert len(seg["delta_rms"]) == len(seg["state_rms"]) == 4 and all(x > 0 and np.isfinite(x) for x in seg["delta_rms"] + seg["state_rms"])
        wav = lambda d: open(os.path.join(tmp, d, n + ".wav"), "rb").read()
        assert wav("a") == wav("b") and wav("a") != wav("c")                   # the estimate changes no sample, the grid does


def test_facade_keeps_its_signature(small, inputs):
    from covomix_amd.acoustic import SolveError
    sd, model = small
    assert model.ode_grid == "uniform" and model.ode_error is False
    plain = _run(model, inputs, 0.7, "heun3", 9)
    model.last_solve_error = None
    y, err = _model_error(model, inputs, 0.7, "heun3", 9, grid="cosine")
    assert isinstance(y, torch.Tensor) and isinstance(err, SolveError) and len(err.grid) == 4 and not torch.equal(y, plain)
    assert _run(model, inputs, 0.7, "heun3", 9).equal(plain) and model.last_solve_error is err            # a plain call leaves the last table alone
