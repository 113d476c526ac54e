"""The flow-matching loss on the GPU: the three kernels of csrc/flow_loss.hip against the existing norm kernel (bit for bit), the numpy
restatement (==) and fp64; one evaluation with a time per utterance against the fp64 oracle where the row count changes route; the
route it takes; a batch above the deferral threshold; the facade (seeds, explicit draws, conditioning drop, placement, launch cuts,
saturation re-run, the regression sample, the tool).

Model: the synthetic state of test_parity_at_size_gpu._state at dim = 512, dim_emb = 64, depth = 4 (skip combiners in layers 2-3),
heads = 8; VoMix and VoSingle alternate.  Bounds: pred against fp64 5e-6 over the batch and 1e-5 per utterance (f16: 1e-3 / 2e-3), the
project's fp32-class bounds of test_acoustic_routes_gpu.py.  The loss: with a = pred - flow and e the error of pred over the masked rows,
|L^ - L| / L <= 2 d + d^2, d = |e| / |a| <= tol |pred| / |pred - flow| (oracle values), plus the reduction bound of the kernel:
(ceil(dim_out / 64) + 8) 2^-24 for a row's mean and (ops.masked_mse_tree_depth(T) + 2) 2^-24 for the sum over the rows (depth =
ceil(T / 256) additions in a thread + 6 in the wave + 2 across the four waves; all terms >= 0, so relative errors add)."""
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

import flow_loss_restated as rs
from conftest import rel_l2
from test_parity_at_size_gpu import _state

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MAIN = dict(dim=512, dim_emb=64, depth=4, heads=8)
KINDS = ("vomix", "vosingle")
TIMES = (0.0, 1.0, 0.31, 0.77)
FP64_TOL, F16_TOL = 5e-6, 1e-3
ROW_BOUND = (math.ceil(80 / 64) + 8) * U

_SD, _MODELS, _ORACLE = {}, {}, {}


def _sd(kind):
    if kind not in _SD:
        sd = _state(kind, **MAIN)
        _SD[kind] = (sd, {k: v.double() for k, v in sd.items()})
    return _SD[kind]


def _model(kind, precision):
    from covomix_amd.conditional_model import CoVoMixModel
    key = (kind, precision)
    if key not in _MODELS:
        _MODELS[key] = CoVoMixModel.from_state_dict(_sd(kind)[0], precision=precision).eval().to("cuda:0")
    return _MODELS[key]


def _utt(kind, T):
    return rs.utterance(kind, T, seed=9000 + T)


def _oracle(kind, T, t, drop=False):
    """fp64 pred / flow / loss of one utterance at one time: computed once, shared by the precisions, left unchanged"""
    key = (kind, T, t, drop)
    if key not in _ORACLE:
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        _ORACLE[key] = rs.oracle_utterance(_sd(kind)[1], _utt(kind, T), t, 0.0, drop)
    return _ORACLE[key]


def _quiet(fn, *a, **k):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*a, **k)
    assert not any("saturat" in str(w.message) for w in rec), [str(w.message)[:100] for w in rec]
    return out


def _loss_call(model, utts, times, **kw):
    return model.flow_matching_loss([u["phoneme_ids"] for u in utts], [u["mel"] for u in utts], cond_mels=[u["cond"] for u in utts],
                                    masks=[u["mask"] for u in utts], times=list(times), x0=[u["x0"] for u in utts], **kw)


# ---------------------------------------------------------------- 1. adarmsnorm_seq == adarmsnorm per sequence
@pytest.mark.parametrize("D", [256, 512, 1024, 1028])
@pytest.mark.parametrize("lengths", [[1, 63, 64, 65, 3], [341, 451, 232]])
def test_adarmsnorm_seq_is_the_norm_of_every_slice(lengths, D):
    from covomix_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(D + len(lengths))
    n, M = len(lengths), sum(lengths)
    tail = 5
    x = (torch.randn(M + tail, D, generator=g) * 3).to(dev)
    table = torch.randn(n, 3, 4, D, generator=g).to(dev)                 # a table with a row stride: rows 12 D floats apart
    gamma, beta = table[:, 1, 0], table[:, 1, 1]
    assert gamma.stride(0) == 12 * D
    rg = ops.Ragged(lengths, dev)
    scale = torch.tensor([4.0], device=dev)
    nan32 = lambda: torch.full((M + tail, D), float("nan"), device=dev)
    nan16 = lambda: torch.full((M + tail, D), float("nan"), dtype=torch.float16, device=dev)
    ops.saturation_reset()
    # fp32 output (with beta and without), the plain pair with a pre-scale, the interleaved pair with a pre-scale
    out, out_nb = nan32(), nan32()
    ops.adarmsnorm_seq(x, gamma, beta, out, rg)
    ops.adarmsnorm_seq(x, gamma, None, out_nb, rg)
    hi, lo = nan16(), nan16()
    ops.adarmsnorm_seq(x, gamma, beta, None, rg, out_split=(hi, lo), split_scale=scale)
    both, bh, bl = nan32(), nan16(), nan16()
    ops.adarmsnorm_seq(x, gamma, beta, both, rg, out_split=(bh, bl), split_scale=scale)
    il = None
    if D % 32 == 0:
        il = ops.SplitIL(M + tail, D, dev)
        il.buf.fill_(float("nan"))
        ops.adarmsnorm_seq(x, gamma, beta, None, rg, out_split=il, split_scale=scale)
    for i in range(n):
        r0, r1 = rg.cu_host[i], rg.cu_host[i + 1]
        xs = x[r0:r1].contiguous()
        want, want_nb = torch.empty_like(xs), torch.empty_like(xs)
        ops.adarmsnorm(xs, gamma[i], beta[i], want)
        ops.adarmsnorm(xs, gamma[i], None, want_nb)
        wh, wl = torch.empty_like(xs, dtype=torch.float16), torch.empty_like(xs, dtype=torch.float16)
        ops.adarmsnorm(xs, gamma[i], beta[i], None, out_split=(wh, wl), split_scale=scale)
        assert torch.equal(out[r0:r1], want) and torch.equal(out_nb[r0:r1], want_nb) and torch.equal(both[r0:r1], want), (i, D)
        assert torch.equal(hi[r0:r1], wh) and torch.equal(lo[r0:r1], wl) and torch.equal(bh[r0:r1], wh) and torch.equal(bl[r0:r1], wl), (i, D)
        if il is not None:
            wil = ops.SplitIL(r1 - r0, D, dev)
            ops.adarmsnorm(xs, gamma[i], beta[i], None, out_split=wil, split_scale=scale)
            assert torch.equal(il.buf[r0:r1], wil.buf), (i, D)
    # rows at or behind cu[n] are not touched
    for t in (out, out_nb, hi, lo, both, bh, bl) + ((il.buf,) if il is not None else ()):
        assert bool(torch.isnan(t[M:]).all()) and bool(torch.isfinite(t[:M]).all())
    assert ops.saturation_query() == 0


def test_adarmsnorm_seq_refusals_leave_the_output_alone():
    from covomix_amd import _lib, ops
    dev = torch.device("cuda:0")
    x, out = torch.randn(12, 64, device=dev), torch.full((12, 64), 7.5, device=dev)
    g = torch.randn(2, 64, device=dev)
    for args in ((x, torch.randn(3, 64, device=dev), None, out, [0, 5, 12]), (x, g, None, out, [0, 5, 13]), (x, g, None, out, [0, 7, 5]),
                 (x, g, g[:, :32], out, [0, 5, 12])):
        with pytest.raises(ValueError):
            ops.adarmsnorm_seq(*args)
    # the C entry point's own checks: a device table is not looked at, the host table is
    lib, cu = _lib.load(), torch.tensor([0, 5, 12], dtype=torch.int32)
    cu_dev = cu.to(dev)
    call = lambda host, n, rows, D=64, stride=64: lib.cvx_adarmsnorm_seq_f32(x.data_ptr(), g.data_ptr(), None, out.data_ptr(), None, None, rows, D,
                                                                             host.data_ptr(), cu_dev.data_ptr(), n, stride, 8.0, 1e-12, None,
                                                                             ops._stream())
    bad_order, bad_end = torch.tensor([0, 9, 5], dtype=torch.int32), torch.tensor([0, 5, 13], dtype=torch.int32)
    for rc in (call(bad_order, 2, 12), call(bad_end, 2, 12), call(cu, 0, 12), call(cu, 4097, 12), call(cu, 2, 12, D=62), call(cu, 2, 12, stride=60),
               call(cu, 2, -1)):
        assert rc == -22
    torch.cuda.synchronize()
    assert bool((out == 7.5).all())
    assert call(cu, 2, 12) == 0
    torch.cuda.synchronize()
    assert bool((out != 7.5).all())


# ---------------------------------------------------------------- 2. cfm_inputs == the restatement
@pytest.mark.parametrize("C", [80, 160])
@pytest.mark.parametrize("sigma", [0.0, 1e-4])
def test_cfm_inputs_equal_the_restatement(sigma, C):
    from covomix_amd import ops
    dev = torch.device("cuda:0")
    lengths = [1, 63, 130, 65, 7]
    times = torch.tensor([0.31, 0.0, 1.0, 0.31, 0.77], dtype=torch.float32)
    g = torch.Generator().manual_seed(C)
    M, tail = sum(lengths), 3
    x1 = (torch.randn(M + tail, 80, generator=g) * 2 - 6)
    x0, cond = torch.randn(M + tail, 80, generator=g), torch.randn(M + tail, C, generator=g) * 3
    mask = torch.rand(M + tail, generator=g) < 0.5                     # mixed ...
    mask[1:64] = True                                                  # ... sequence 1 all true, sequence 2 all false
    mask[64:194] = False
    rg = ops.Ragged(lengths, dev)
    w = torch.full((M + tail, 80), float("nan"), device=dev)
    flow, cond_in = torch.full_like(w, float("nan")), torch.full((M + tail, C), float("nan"), device=dev)
    ops.cfm_inputs(x1.to(dev), x0.to(dev), cond.to(dev), mask.to(dev), times.to(dev), rg, sigma, w, flow, cond_in)
    rows_t = np.repeat(times.numpy(), lengths)
    rw, rf, rc = rs.cfm_inputs(x1[:M].numpy(), x0[:M].numpy(), cond[:M].numpy(), mask[:M].numpy(), rows_t, sigma)
    assert (w[:M].cpu().numpy() == rw).all() and (flow[:M].cpu().numpy() == rf).all() and (cond_in[:M].cpu().numpy() == rc).all()
    for t in (w, flow, cond_in):
        assert bool(torch.isnan(t[M:]).all())
    # uint8 masks are bools; a fresh flow / cond_in is allocated when none is passed
    w2 = torch.empty(M + tail, 80, device=dev)
    _, f2, c2 = ops.cfm_inputs(x1.to(dev), x0.to(dev), cond.to(dev), mask.to(torch.uint8).to(dev), times.to(dev), rg, sigma, w2)
    assert torch.equal(w2[:M], w[:M]) and torch.equal(f2[:M], flow[:M]) and torch.equal(c2[:M], cond_in[:M])
    # refusals leave the outputs alone
    keep = w.clone()
    with pytest.raises(ValueError):
        ops.cfm_inputs(x1.to(dev), x0.to(dev), cond.to(dev), mask.to(dev), times[:4].to(dev), rg, sigma, w, flow, cond_in)
    with pytest.raises(ValueError):
        ops.cfm_inputs(x1.to(dev), x0.to(dev), cond.to(dev), mask.to(dev), times.to(dev), [0, 5, M + tail + 1], sigma, w, flow, cond_in)
    assert torch.equal(torch.nan_to_num(w), torch.nan_to_num(keep))


# ---------------------------------------------------------------- 3. masked_mse
def test_masked_mse_rows_sums_counts_and_placement():
    from covomix_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(17)
    lengths = [1, 300, 257, 64, 1030]
    seqs = [dict(pred=torch.randn(T, 80, generator=g) * 2, flow=torch.randn(T, 80, generator=g), mask=torch.rand(T, generator=g) < 0.6)
            for T in lengths]
    seqs[3]["mask"][:] = False                                          # an empty mask: loss 0, count 0
    seqs[0]["mask"][:] = True

    def pool(order, gaps):
        """the sequences in `order`, `gaps[k]` NaN rows in front of the k-th (and 4 behind the last): offsets and the row tensors"""
        pred, flow, mask, cu = [], [], [], []
        for k, i in enumerate(order):
            for lst, fill in ((pred, float("nan")), (flow, float("nan"))):
                lst.append(torch.full((gaps[k], 80), fill))
            mask.append(torch.ones(gaps[k], dtype=torch.bool))
            cu.append(sum(t.shape[0] for t in mask))
            pred.append(seqs[i]["pred"]); flow.append(seqs[i]["flow"]); mask.append(seqs[i]["mask"])
        end = sum(t.shape[0] for t in mask)
        pred.append(torch.full((4, 80), float("nan"))); flow.append(torch.full((4, 80), float("nan"))); mask.append(torch.ones(4, dtype=torch.bool))
        return torch.cat(pred).to(dev), torch.cat(flow).to(dev), torch.cat(mask).to(dev), cu, end

    # packed back to back (offsets n + 1): every sequence
    pred, flow, mask, cu, end = pool(range(5), [0] * 5)
    err0 = torch.full((end + 4,), float("nan"), device=dev)
    loss, count, err = ops.masked_mse(pred, flow, mask, cu + [end], err_rows=err0)
    assert err is err0 and bool(torch.isnan(err[end:]).all())
    loss, count, err = loss.cpu(), count.cpu(), err.cpu()
    worst_row = worst_sum = 0.0
    for i, T in enumerate(lengths):
        s = seqs[i]
        e64 = (s["pred"].double() - s["flow"].double()).square().mean(-1)
        e = err[cu[i]:cu[i] + T].double()
        worst_row = max(worst_row, float(((e - e64).abs() / e64).max()))
        assert bool(((e - e64).abs() <= ROW_BOUND * e64).all()), i
        m = s["mask"]
        assert int(count[i]) == int(m.sum())
        num64 = float(e[m].sum())                                       # the fp64 sum of the kernel's OWN row errors
        want = num64 / max(float(m.sum()), 1e-5)
        depth = ops.masked_mse_tree_depth(T)                            # ceil(T / 256) + 6 + 2; + 1 for the division, + 1 spare: depth + 2
        assert depth == math.ceil(T / 256) + 8
        if m.any():
            rel = abs(float(loss[i]) - want) / want
            worst_sum = max(worst_sum, rel / ((depth + 2) * U))
            assert rel <= (depth + 2) * U, (i, rel)
        else:
            assert float(loss[i]) == 0.0 and int(count[i]) == 0
    print(f"FIGURE masked_mse worst row error {worst_row / U:.2f} x 2^-24 (bound {ROW_BOUND / U:.0f}), worst sequence sum at {worst_sum:.2f} of its bound")
    # moved, other neighbours, NaN rows between the sequences (masked True there: a row outside a sequence is never read into a sum)
    pred2, flow2, mask2, cu2, end2 = pool([4, 2, 1], [3, 1, 7])
    for k, i in enumerate([4, 2, 1]):
        l2, c2, e2 = ops.masked_mse(pred2, flow2, mask2, [cu2[k], cu2[k] + lengths[i]])
        assert torch.equal(l2.cpu(), loss[i:i + 1]) and int(c2) == int(count[i])
        assert torch.equal(e2[cu2[k]:cu2[k] + lengths[i]].cpu(), err[cu[i]:cu[i] + lengths[i]])
        assert bool((e2[:cu2[k]] == 0).all()) and bool((e2[cu2[k] + lengths[i]:] == 0).all())       # a fresh err_rows: zero elsewhere
    # a table with an empty sequence between two others
    l3, c3, _ = ops.masked_mse(pred, flow, mask, [cu[1], cu[2], cu[2], cu[3]])
    assert torch.equal(l3.cpu()[[0, 2]], loss[1:3]) and float(l3[1]) == 0.0 and c3.tolist() == [int(count[1]), 0, int(count[2])]


# ---------------------------------------------------------------- 4. / 5. one evaluation with a time per utterance
CASES = [[37, 27], [37, 28], [69, 58], [69, 59], [341, 451, 232], [685, 901, 462]]


def _case_params():
    out = []
    for n, lengths in enumerate(CASES):
        for p in ("f16x3", "fp32") + (("f16",) if lengths == [341, 451, 232] else ()):
            out.append(pytest.param(KINDS[n % 2], lengths, p, id=f"M{sum(lengths)}-{KINDS[n % 2]}-{p}"))
    return out


class _Recorder:
    KEYS = ("gemm", "gemm_norm", "gemm_rowsq", "adarmsnorm", "adarmsnorm_seq", "rownorm_scale", "deferred_tables")

    def __init__(self, monkeypatch):
        import covomix_amd.acoustic as ac
        import covomix_amd.ops as ops_
        self.n = n = dict.fromkeys(self.KEYS, 0)
        real_gemm = ops_.gemm

        def gemm(a, w, out, **k):
            n["gemm"] += 1
            n["gemm_norm"] += k.get("norm") is not None
            n["gemm_rowsq"] += k.get("c_rowsq") is not None or k.get("a_row_scale") is not None
            return real_gemm(a, w, out, **k)
        monkeypatch.setattr(ops_, "gemm", gemm)

        def through(obj, name, key):
            real = getattr(obj, name)

            def fn(*a, **k):
                n[key] += 1
                return real(*a, **k)
            monkeypatch.setattr(obj, name, fn)
        for name in ("adarmsnorm", "adarmsnorm_seq", "rownorm_scale"):
            through(ops_, name, name)
        through(ac.VectorField, "_deferred_norm_tables", "deferred_tables")


@pytest.mark.parametrize("kind,lengths,precision", _case_params())
def test_evaluation_with_a_time_per_utterance(kind, lengths, precision, monkeypatch):
    import dataclasses
    from covomix_amd import ops
    from covomix_amd.acoustic import route, route_seq_times
    M, times = sum(lengths), TIMES[:len(lengths)]
    utts = [_utt(kind, T) for T in lengths]
    model = _model(kind, precision)
    rec = _Recorder(monkeypatch)
    res = _quiet(_loss_call, model, utts, times, return_pred=True)
    # 5. the route: route()'s record of the row count with the three forms off; two per-sequence norms per layer, the final norm alone on
    # the one-row kernel, no norm inside a GEMM, no deferred-norm machinery, no graph
    r = route_seq_times(M, MAIN["dim"], precision, M)
    assert r == dataclasses.replace(route(M, MAIN["dim"], precision, M), fuse_norm=False, deferred=False, graph=False)
    assert r.split_io == (precision != "fp32" and M > 64) and r.interleaved == (precision == "f16x3" and M >= ops.il_min_rows())
    n = rec.n
    assert n["adarmsnorm_seq"] == 2 * MAIN["depth"] and n["adarmsnorm"] == 1, n
    assert n["gemm_norm"] == n["gemm_rowsq"] == n["rownorm_scale"] == n["deferred_tables"] == 0, n
    assert not model._get_field().__dict__.get("_graphs")
    ws = model._get_field()._ws[("ragged", r.ragged_capacity, M >= ops.il_min_rows())]
    assert isinstance(ws.get("normed16"), ops.SplitIL) == r.interleaved
    # 4. every utterance against its own B = 1 fp64 run at ITS time (a neighbour's gamma would show: the times are far apart)
    refs = [_oracle(kind, T, t) for T, t in zip(lengths, times)]
    tol = F16_TOL if precision == "f16" else FP64_TOL
    e_all = rel_l2(torch.cat(res.pred), torch.cat([r_["pred"] for r_ in refs]))
    worst = max(rel_l2(p, r_["pred"]) for p, r_ in zip(res.pred, refs))
    assert [tuple(p.shape) for p in res.pred] == [(T, 80) for T in lengths] and all(bool(torch.isfinite(p).all()) for p in res.pred)
    figures = []
    for i, (u, ref, T) in enumerate(zip(utts, refs, lengths)):
        m = u["mask"]
        d = 2 * tol * float(ref["pred"][m].norm()) / float((ref["pred"][m] - ref["flow"][m]).norm())
        bound = 2 * d + d * d + ROW_BOUND + (ops.masked_mse_tree_depth(T) + 2) * U
        rel = abs(float(res.per_utterance[i]) - ref["loss"]) / ref["loss"]
        figures.append(f"{rel:.2e}/{bound:.2e}")
        assert int(res.frames[i]) == int(m.sum())
        assert rel <= bound, (i, rel, bound, float(res.per_utterance[i]), ref["loss"])
        # the facade's own numbers agree with each other: the loss is the masked mean of the row errors it returns
        own = float(res.err_rows[i].double()[m].sum() / float(m.sum()))
        assert abs(float(res.per_utterance[i]) - own) <= (ops.masked_mse_tree_depth(T) + 2) * U * own
    print(f"FIGURE flow-loss {kind} {precision} lengths={lengths} M={M} pred_err_vs_fp64={e_all:.3e} worst_utterance={worst:.3e} "
          f"loss_err/bound={figures} losses={[round(float(x), 4) for x in res.per_utterance]}")
    assert e_all <= tol and worst <= 2 * tol, (e_all, worst)
    assert abs(res.loss - float(res.per_utterance.mean())) == 0.0 and res.per_utterance.dtype == torch.float64
    assert torch.equal(res.times, torch.tensor(times, dtype=torch.float32))


MANY = [5 + (7 * i) % 41 for i in range(40)]           # 40 utterances of 5 ... 45 frames (960 rows): more than the 32 times the skinny GEMM takes


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_forty_utterances_take_the_tiled_table_gemm(precision):
    """Above 32 utterance times _time_tables leaves cvx_gemm_skinny_f32: the time MLP and the adaptive-norm table come from the tiled GEMM
    (f16x3: the split GEMM on split_act_f16(temb)).  40 utterances, times spread over [0, 1] with both ends, every utterance against its
    own B = 1 fp64 run at the bounds of the cases above."""
    from covomix_amd import ops
    kind, lengths = "vosingle", MANY
    times = [0.0, 1.0] + [round((i * 0.6180339887) % 1.0, 4) for i in range(2, 40)]
    utts = [rs.utterance(kind, T, seed=500 + i) for i, T in enumerate(lengths)]
    res = _quiet(_loss_call, _model(kind, precision), utts, times, return_pred=True)
    sd64 = _sd(kind)[1]
    refs = [rs.oracle_utterance(sd64, u, t) for u, t in zip(utts, times)]
    e_all = rel_l2(torch.cat(res.pred), torch.cat([r["pred"] for r in refs]))
    worst = max(rel_l2(p, r["pred"]) for p, r in zip(res.pred, refs))
    worst_loss = 0.0
    for i, (u, ref, T) in enumerate(zip(utts, refs, lengths)):
        m = u["mask"]
        d = 2 * FP64_TOL * float(ref["pred"][m].norm()) / float((ref["pred"][m] - ref["flow"][m]).norm())
        bound = 2 * d + d * d + ROW_BOUND + (ops.masked_mse_tree_depth(T) + 2) * U
        rel = abs(float(res.per_utterance[i]) - ref["loss"]) / ref["loss"]
        worst_loss = max(worst_loss, rel / bound)
        assert rel <= bound, (i, T, times[i], rel, bound)
    print(f"FIGURE flow-loss 40 utterances {precision} M={sum(lengths)} pred_err_vs_fp64={e_all:.3e} worst_utterance={worst:.3e} "
          f"worst loss error at {worst_loss:.3f} of its bound")
    assert e_all <= FP64_TOL and worst <= 2 * FP64_TOL, (e_all, worst)


# ---------------------------------------------------------------- 6. above the deferral threshold
def test_above_the_deferral_threshold_runs_without_deferred_tables(monkeypatch):
    import covomix_amd.acoustic as ac
    lengths, kind = [2731, 2731, 2731], "vosingle"                      # 8193 rows
    assert ac.route(8193, MAIN["dim"], "f16x3", 8193).deferred and not ac.route_seq_times(8193, MAIN["dim"], "f16x3", 8193).deferred

    def refuse(*a, **k):
        raise AssertionError("an evaluation with a time per sequence must not build deferred-norm tables")
    monkeypatch.setattr(ac.VectorField, "_deferred_norm_tables", refuse)
    utts = [_utt(kind, T + i) for i, T in enumerate([2731, 2730, 2732])]
    a = _quiet(_loss_call, _model(kind, "f16x3"), utts, TIMES[:3], return_pred=True)
    b = _quiet(_loss_call, _model(kind, "fp32"), utts, TIMES[:3], return_pred=True)
    e = rel_l2(torch.cat(a.pred), torch.cat(b.pred))
    worst = max(rel_l2(x, y) for x, y in zip(a.pred, b.pred))
    rel = float(((a.per_utterance - b.per_utterance).abs() / b.per_utterance).max())
    print(f"FIGURE flow-loss 8193 rows f16x3 against the fp32 field: pred {e:.3e} worst utterance {worst:.3e} loss {rel:.3e}")
    assert e <= FP64_TOL and worst <= 2 * FP64_TOL
    for i, u in enumerate(utts):
        m = u["mask"]
        d = 2 * FP64_TOL * float(b.pred[i][m].norm()) / float((b.pred[i][m] - (u["mel"] - u["x0"])[m]).norm())
        assert abs(float(a.per_utterance[i] - b.per_utterance[i])) / float(b.per_utterance[i]) <= 2 * d + d * d + 2 * (ROW_BOUND + 21 * U)


# ---------------------------------------------------------------- 7. the facade
def test_facade_seeds_explicit_draws_and_launch_cuts():
    from covomix_amd import flow_loss as fl
    kind, lengths = "vosingle", [37, 91, 64, 120]
    utts = [_utt(kind, T) for T in lengths]
    model = _model(kind, "f16x3")
    ids, mels = [u["phoneme_ids"] for u in utts], [u["mel"] for u in utts]
    a, b = _quiet(model.flow_matching_loss, ids, mels, seed=11), _quiet(model.flow_matching_loss, ids, mels, seed=11)
    assert a.loss == b.loss and torch.equal(a.per_utterance, b.per_utterance) and torch.equal(a.times, b.times)
    assert all(torch.equal(x, y) for x, y in zip(a.err_rows + a.masks, b.err_rows + b.masks))
    c = _quiet(model.flow_matching_loss, ids, mels, seed=12)
    assert not torch.equal(a.times, c.times) and a.loss != c.loss
    # the documented draws, passed explicitly, reproduce the seeded call bit for bit (cond_mels defaults to mels)
    dr = fl.draw(lengths, 80, 11)
    e = _quiet(model.flow_matching_loss, ids, mels, cond_mels=mels, masks=dr["masks"], times=dr["times"], x0=dr["x0"])
    assert torch.equal(e.per_utterance, a.per_utterance) and all(torch.equal(x, y) for x, y in zip(e.err_rows, a.err_rows))
    assert all(torch.equal(x, y) for x, y in zip(a.masks, dr["masks"]))
    # cut into launches of at most 128 rows ([37, 91], [64], [120]): the same mean within 1e-6 relative
    cut = _quiet(model.flow_matching_loss, ids, mels, seed=11, max_rows=128)
    print(f"FIGURE flow-loss facade loss {a.loss:.6f}, cut into three launches {cut.loss:.6f}, rel {abs(cut.loss - a.loss) / a.loss:.2e}")
    assert abs(cut.loss - a.loss) <= 1e-6 * a.loss
    # an empty mask is no error: 0 through the clamp
    z = _quiet(model.flow_matching_loss, ids[:2], mels[:2], masks=[torch.zeros(37, dtype=torch.bool), utts[1]["mask"]], seed=3)
    assert float(z.per_utterance[0]) == 0.0 and int(z.frames[0]) == 0 and float(z.per_utterance[1]) > 0


def test_facade_placement_among_other_neighbours():
    """An utterance's result is bit-identical at another place among other neighbours in a batch of the same row count: first of
    [91, 64, 93] and second of [64, 91, 93] (other utterances, other times).  Every new kernel is row-local and takes a sequence's rows
    in place, so its part holds at ANY offset (test_masked_mse_rows_sums_counts_and_placement moves sequences by 1, 3 and 7 rows); the
    network in between holds it where the split-precision attention tiles the keys alike: that kernel keeps its key tiles aligned to 32
    packed rows, so the two places here are 64 rows apart.  At an offset that is no multiple of 32 (third of [93, 64, 91]:
    row 157) the keys fall into other tiles and the result agrees up to fp32 summation order, as every ragged solve's does: both are
    within 1e-5 of the truth, so within 2e-5 of each other (asserted; the figure is printed)."""
    kind = "vomix"
    model = _model(kind, "f16x3")
    u = _utt(kind, 91)
    other = lambda T, seed: rs.utterance(kind, T, seed=seed)
    first = _quiet(_loss_call, model, [u, other(64, 1), other(93, 2)], (0.31, 0.0, 1.0), return_pred=True)
    second = _quiet(_loss_call, model, [other(64, 3), u, other(93, 4)], (0.77, 0.31, 0.0), return_pred=True)
    assert torch.equal(first.pred[0], second.pred[1]) and torch.equal(first.err_rows[0], second.err_rows[1])
    assert float(first.per_utterance[0]) == float(second.per_utterance[1]) and int(first.frames[0]) == int(second.frames[1])
    third = _quiet(_loss_call, model, [other(93, 5), other(64, 6), u], (1.0, 0.77, 0.31), return_pred=True)
    e = rel_l2(third.pred[2], first.pred[0])
    rel = abs(float(third.per_utterance[2] - first.per_utterance[0])) / float(first.per_utterance[0])
    print(f"FIGURE flow-loss placement: rows 0 and 64 bit-identical; row 157 (other key tiles) pred {e:.3e}, loss {rel:.3e}, "
          f"equal bits: {torch.equal(third.pred[2], first.pred[0])}")
    assert e <= 4 * FP64_TOL


def test_facade_cond_drop_is_the_call_with_null_inputs():
    kind, lengths, times = "vosingle", [69, 59], (0.31, 0.77)
    utts = [_utt(kind, T) for T in lengths]
    model = _model(kind, "f16x3")
    res = _quiet(_loss_call, model, utts, times, cond_drop=[True, False], return_pred=True)
    keep = _quiet(_loss_call, model, utts, times, return_pred=True)
    # the kept utterance is untouched by its neighbour's drop; the dropped one runs on the null phoneme id and null_cond: the oracle's
    # drop_cond branch at B = 1
    assert torch.equal(res.pred[1], keep.pred[1]) and not torch.equal(res.pred[0], keep.pred[0])
    ref = _oracle(kind, lengths[0], times[0], drop=True)
    e = rel_l2(res.pred[0], ref["pred"])
    moved = abs(float(res.per_utterance[0] - keep.per_utterance[0])) / float(keep.per_utterance[0])
    print(f"FIGURE flow-loss cond_drop pred_err_vs_fp64={e:.3e}; dropping the conditioning moves the loss by {moved:.2e}")
    assert e <= 2 * FP64_TOL
    m = utts[0]["mask"]
    d = 2 * FP64_TOL * float(ref["pred"][m].norm()) / float((ref["pred"][m] - ref["flow"][m]).norm())
    assert abs(float(res.per_utterance[0]) - ref["loss"]) / ref["loss"] <= 2 * d + d * d + ROW_BOUND + 11 * U
    # the same through the field: null ids and null_cond rows given as the inputs
    field, d_ = model._get_field(), model._get_field().d
    from covomix_amd import ops
    dev = field.device
    rg = ops.Ragged(lengths, dev)
    cat = lambda k: torch.cat([u[k] for u in utts]).to(dev)
    t_d = torch.tensor(times, device=dev)
    w, flow, cond_in = ops.cfm_inputs(cat("mel"), cat("x0"), cat("cond"), cat("mask"), t_d, rg, 0.0, field.xin_rows(lengths))
    cond_in[:lengths[0]] = field.sd["null_cond"]
    ids = cat("phoneme_ids").clone()
    ids[:lengths[0]] = d_["null_id"]
    pred = field.evaluate_seq_times(ids, cond_in, w, t_d, lengths)
    assert torch.equal(pred[:lengths[0]].cpu(), res.pred[0]) and torch.equal(pred[lengths[0]:].cpu(), res.pred[1])


def test_facade_saturation_rerun(monkeypatch):
    """The saturation contract of synthesis_sample: one weight row times 2^14 (as test_saturation_gpu.py scales it) is never silently
    wrong, and an input far outside the window is re-run on the fp32 field (or raises) with the same draws."""
    from covomix_amd._lib import CovomixHipError
    from covomix_amd.conditional_model import CoVoMixModel
    kind, lengths, times = "vosingle", [69, 59], (0.31, 0.77)
    utts = [_utt(kind, T) for T in lengths]
    sd = dict(_sd(kind)[0])
    sd["to_embed.weight"] = sd["to_embed.weight"].clone()
    sd["to_embed.weight"][77] *= 2.0 ** 14
    split = CoVoMixModel.from_state_dict(sd, precision="f16x3").eval().to("cuda:0")
    exact = CoVoMixModel.from_state_dict(sd, precision="fp32").eval().to("cuda:0")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a = _loss_call(split, utts, times, return_pred=True)
    rerun = any("saturat" in str(w.message) for w in rec)
    b = _loss_call(exact, utts, times, return_pred=True)
    e = rel_l2(torch.cat(a.pred), torch.cat(b.pred))
    print(f"FIGURE flow-loss outlier row x 2^14: against the fp32 field {e:.3e} ({'flagged -> fp32 re-run' if rerun else 'inside the window'})")
    assert e <= 2 * FP64_TOL and bool(torch.isfinite(a.per_utterance).all())
    # far outside: the conditioning mel times 4000
    far = [dict(u, cond=u["cond"] * 4000.0) for u in utts]
    model, ref = _model(kind, "f16x3"), _loss_call(_model(kind, "fp32"), far, times, return_pred=True)
    with pytest.warns(UserWarning, match="saturat"):
        out = _loss_call(model, far, times, return_pred=True)
    # (both are runs of the fp32 kernels on the same inputs and draws)
    assert rel_l2(torch.cat(out.pred), torch.cat(ref.pred)) <= FP64_TOL
    assert float(((out.per_utterance - ref.per_utterance).abs() / ref.per_utterance).max()) <= 1e-5
    monkeypatch.setenv("CVX_ON_SATURATION", "raise")
    with pytest.raises(CovomixHipError, match="saturat"):
        _loss_call(model, far, times)
    monkeypatch.delenv("CVX_ON_SATURATION")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _loss_call(model, utts, times)               # a normal input right afterwards is neither flagged nor re-run


def test_regression_sample_against_the_oracle():
    import covomix_oracle as orc
    import covomix_amd.synthetic as syn
    kind, B, T, s = "vomix", 2, 48, 0.7
    sd, sd64 = _sd(kind)
    inp = syn.synthetic_inputs(kind, B, T, 16, seed=77)
    times = [0.31, 0.77]
    model = _model(kind, "f16x3")
    out = _quiet(model.synthesis_regression_duration, inp["phoneme_ids"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), s, y0=inp["y0"], times=times)
    ref = orc.forward_with_cond_scale(sd64, inp["y0"].double(), torch.tensor(times, dtype=torch.float32).double(), inp["phoneme_ids"],
                                      inp["cond"].double(), s)
    e, worst = rel_l2(out, ref), max(rel_l2(out[b], ref[b]) for b in range(B))
    assert out.shape == (B, T, 80) and out.is_cuda
    # lists of different lengths, scale 1 (the conditional branch alone): each against its own B = 1 oracle run
    us = [{k: v[0] for k, v in syn.synthetic_inputs(kind, 1, L, L // 3, seed=80 + L).items()} for L in (33, 70)]
    outs = _quiet(model.synthesis_regression_duration, [u["phoneme_ids"] for u in us], [u["cond"] for u in us], None, 1.0,
                  y0=[u["y0"] for u in us], times=times)
    refs = [orc.forward_with_cond_scale(sd64, u["y0"][None].double(), torch.tensor([t], dtype=torch.float32).double(), u["phoneme_ids"][None],
                                        u["cond"][None].double(), 1.0)[0] for u, t in zip(us, times)]
    e1 = max(rel_l2(o, r) for o, r in zip(outs, refs))
    print(f"FIGURE regression sample scale {s}: err_vs_fp64={e:.3e} worst item {worst:.3e}; lists at scale 1: worst {e1:.3e}")
    assert e <= FP64_TOL and worst <= 2 * FP64_TOL and e1 <= 2 * FP64_TOL
    assert [tuple(o.shape) for o in outs] == [(33, 80), (70, 80)]
    # drawn noise and times: finite, and another call draws other ones
    r1 = model.synthesis_regression_duration(inp["phoneme_ids"].cuda(), inp["cond"].cuda(), None, s)
    r2 = model.synthesis_regression_duration(inp["phoneme_ids"].cuda(), inp["cond"].cuda(), None, s)
    assert bool(torch.isfinite(r1).all()) and not torch.equal(r1, r2)


def test_tool_end_to_end(tmp_path):
    import importlib.util
    import covomix_amd.synthetic as syn
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("eval_flow_loss", os.path.join(ROOT, "tools", "eval_flow_loss.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    shapes = syn.acoustic_param_shapes(dim=128, dim_cond=80, dim_emb=64, depth=2, heads=2, streams=1)
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed=0).items()}
    ckpt = tmp_path / "model.ckpt"
    torch.save({"state_dict": {"cfm_wrapper.CoVoMix." + k: v for k, v in sd.items()}}, ckpt)
    mel, tok = tmp_path / "mel", tmp_path / "tok"
    mel.mkdir(), tok.mkdir()
    for name, T in (("a", 40), ("b", 75), ("c", 33)):
        u = rs.utterance("vosingle", T, seed=T)
        np.save(mel / f"{name}.mel.npy", u["mel"].t().contiguous().numpy())
        if name != "c":
            np.save(tok / f"{name}.semantic.npy", u["phoneme_ids"].numpy())
    out = tmp_path / "out.json"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert tool.main(["--ckpt", str(ckpt), "--mel_dir", str(mel), "--token_dir", str(tok), "--json", str(out), "--seed", "4", "--draws", "2"]) == 0
        res = json.load(open(out))
        assert res["utterances"] == ["a", "b"] and res["frames"] == [40, 75] and res["missing"]["no_tokens"] == ["c"] and res["draws"] == 2
        assert len(res["per_utterance"]) == 2 and all(math.isfinite(x) and x > 0 for x in res["per_utterance"])
        assert abs(res["loss"] - sum(res["per_utterance"]) / 2) < 1e-12 and "random-weight" in res["note"]
        assert tool.main(["--ckpt", str(ckpt), "--mel_dir", str(mel), "--token_dir", str(tok), "--json", str(out), "--times", "0,0.5,1"]) == 0
        curve = json.load(open(out))["curve"]
    assert [c["time"] for c in curve] == [0.0, 0.5, 1.0] and all(math.isfinite(c["loss"]) and c["loss"] > 0 for c in curve)
