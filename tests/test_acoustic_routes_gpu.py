"""The acoustic solve against an fp64 evaluation of the oracle at the row counts where VectorField.evaluate changes route.

One evaluation of the network has M rows (B T at cond_scale 1, 2 B T with the null branch, the packed lengths for a ragged batch), and
the host code picks its kernels from M: fp32 kernels up to 64 rows, the split pipe on plain (hi, lo) pairs up to 127, interleaved pairs
from 128, norms fused into their producers below 2048, the split-K scratch up to 2048, deferred norms from 8192, no captured graph past
8192; a ragged workspace grows in steps of 1024 rows.  tests/acoustic_routes.py restates that table (tests/test_acoustic_routes.py holds
it to the library on the CPU); every case here sits ON a boundary or one step beside it, at a width (dim = 512: the narrowest model
with interleaved weights and the deferred path) where the routes really differ, and asserts

  1. the route taken: recording pass-throughs around ops.gemm / adarmsnorm / rownorm_scale / attention / attention_f16x3 (and the
     split-K scratch hand-over) over one eager pass must count what acoustic_routes.expected_record says for the route the case names;
  2. rel-L2 against the fp64 oracle <= 5e-6 for f16x3 and fp32 (the project's fp32-class bound against fp64: test_deferred_norm_is_
     scale_free, test_split_precision_is_scale_free; the fp32 CPU oracle itself sits 6.4e-7 to 7.4e-7 from fp64 on these shapes),
     twice that per utterance, 1e-3 for f16; finite output of the right shape;
  3. a FIGURE line: the error and its ratio to the fp32 oracle's own distance from fp64 (printed, not bounded);
  4. replay: the second call of a graphed case equals the first bit for bit; one model object runs all cases of a crossing, then the
     first again, bit for bit (graph replay and re-capture after eviction, workspace eviction, a smaller ragged batch in a capacity
     workspace a larger one used);
  5. one utterance solved on three routes (B = 3: fused norms; B = 4: stand-alone norms, no scratch; packed first in a ragged batch of
     2048 rows: scratch without fused norms) agrees element by element;
  6. a ragged batch that does not fill its capacity leaves the rows behind it untouched.

Model: the synthetic state of test_parity_at_size_gpu._state at dim = 512, dim_emb = 64, depth = 4 (skip combiners in layers 2-3),
heads = 8; for the 2048-row crossing also dim = 1024, depth = 2, heads = 16 (dim_emb = 64), whose fused norms ride in
splitk_reduce_norm_kernel<4> instead of <2>.  nfe = 2: one midpoint step.  Cases alternate VoMix and VoSingle."""
import dataclasses
import warnings

import pytest
import torch

from acoustic_routes import expected_record, route
from conftest import rel_l2
from test_parity_at_size_gpu import _state

pytestmark = pytest.mark.gpu

NFE = 2
FP64_TOL = 5e-6                     # f16x3 and fp32 against the fp64 oracle (per utterance: twice)
F16_ROLL_TOL = 1e-3                 # 'f16': hi halves only
MAIN = dict(dim=512, dim_emb=64, depth=4, heads=8)
WIDE = dict(dim=1024, dim_emb=64, depth=2, heads=16)
KINDS = ("vomix", "vosingle")

# crossing -> (B, T, cond_scale): M = B T at scale 1.0, 2 B T otherwise
CROSSINGS = {
    "64|65": [(1, 32, 0.7), (1, 65, 1.0), (1, 33, 0.7)],                                                        # 64, 65, 66
    "127|128": [(1, 127, 1.0), (1, 64, 0.7), (1, 129, 1.0)],                                                    # 127, 128, 129
    "2047|2048|2049": [(1, 1023, 0.7), (1, 2047, 1.0), (1, 1024, 0.7), (2, 1024, 1.0), (3, 683, 1.0)],          # 2046, 2047, 2048, 2048, 2049
    "8190|8192|8194": [(3, 1365, 0.7), (4, 1024, 0.7), (17, 241, 0.7)],                                         # default DEFER_MIN_ROWS and graph limit
}
WIDE_CASES = [(1, 1023, 0.7), (1, 1024, 0.7), (3, 683, 1.0)]                                                   # 2046, 2048, 2049
# ragged: distinct lengths, the first with T % 4 == 1; sums of 64 / 65, 127 / 128 (scale 1.0), 1023 / 1024 / 1025 (0.7: M = 2046 in a
# capacity of 2048, 2048 exactly full, 2050 in 3072), 2047 / 2049 (1.0), 4095 / 4096 / 4097 (0.7: M = 8190 / 8192 / 8194)
RAGGED = {
    "r64|65": [([37, 27], 1.0), ([37, 28], 1.0)],
    "r127|128": [([69, 58], 1.0), ([69, 59], 1.0)],
    "r2046|2048|2050": [([341, 450, 232], 0.7), ([341, 451, 232], 0.7), ([341, 452, 232], 0.7)],
    "r2047|2049": [([685, 901, 461], 1.0), ([685, 903, 461], 1.0)],
    "r8190|8192|8194": [([1365, 1801, 929], 0.7), ([1365, 1802, 929], 0.7), ([1365, 1803, 929], 0.7)],
    "r-per-utterance": [([341, 451, 232], (0.7, 1.0, 0.4))],
}


def _rows(B, T, s):
    return B * T * (1 if s == 1.0 else 2)


def _equal_params():
    out, n = [], 0
    for name, cases in CROSSINGS.items():
        precisions = ("f16x3", "fp32", "f16") if name in ("64|65", "2047|2048|2049") else ("f16x3",)
        for case in cases:
            for p in precisions:
                out.append(pytest.param("main", KINDS[n % 2], case, p, id=f"{name}-M{_rows(*case)}-{case[0]}x{case[1]}-{KINDS[n % 2]}-{p}"))
            n += 1
    for case in WIDE_CASES:
        out.append(pytest.param("wide", KINDS[n % 2], case, "f16x3", id=f"wide-M{_rows(*case)}-{case[0]}x{case[1]}-{KINDS[n % 2]}-f16x3"))
        n += 1
    return out


def _ragged_params():
    out, n = [], 0
    for name, cases in RAGGED.items():
        for lengths, s in cases:
            out.append(pytest.param(KINDS[n % 2], lengths, s, id=f"{name}-{sum(lengths)}-{KINDS[n % 2]}"))
            n += 1
    return out


# ---------------------------------------------------------------- states, inputs and references (made once, shared, left unchanged)
_SD, _REF = {}, {}


def _sd(width, kind):
    key = (width, kind)
    if key not in _SD:
        sd = _state(kind, **(MAIN if width == "main" else WIDE))
        _SD[key] = (sd, {k: v.double() for k, v in sd.items()})
    return _SD[key]


def _comb_layers(sd):
    return [i for i in range(64) if f"transformer.layers.{i}.0.weight" in sd]


def _inputs(kind, B, T):
    import covomix_amd.synthetic as syn
    return syn.synthetic_inputs(kind, B, T, T // 3, seed=1000 * B + T)


def _utt(kind, T):
    import covomix_amd.synthetic as syn
    return {k: v[0] for k, v in syn.synthetic_inputs(kind, 1, T, max(1, T // 3), seed=7000 + T).items()}


def _reference(width, kind, inp, s, key):
    """(fp64 oracle, rel-L2 of the fp32 oracle against it) of one solve; cached by case, so the three precisions share it"""
    import covomix_oracle as orc
    key = (width, kind) + key
    if key not in _REF:
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        sd, sd64 = _sd(width, kind)
        ref64 = orc.sample(sd64, inp["phoneme_ids"], inp["cond"].double(), inp["y0"].double(), s, nfe=NFE)
        ref32 = orc.sample(sd, inp["phoneme_ids"], inp["cond"], inp["y0"], s, nfe=NFE)
        _REF[key] = (ref64, ref32)
    return _REF[key]


def _utt_reference(kind, T, s):
    u = _utt(kind, T)
    r64, r32 = _reference("main", kind, {k: v[None] for k, v in u.items()}, s, ("utt", T, s))
    return r64[0], r32[0]


def _model(width, kind, precision):
    from covomix_amd.conditional_model import CoVoMixModel
    return CoVoMixModel.from_state_dict(_sd(width, kind)[0], nfe=NFE, precision=precision).eval().to("cuda:0")


def _solve(model, inp, s):
    return model.synthesis_sample(inp["phoneme_ids"].cuda(), inp["cond"].cuda(), inp["mask"].cuda(), s, y0=inp["y0"])


def _solve_ragged(model, utts, s):
    return model.synthesis_sample([u["phoneme_ids"].cuda() for u in utts], [u["cond"].cuda() for u in utts], None,
                                  list(s) if isinstance(s, tuple) else s, y0=[u["y0"] for u in utts])


class _Recorder:
    """Recording pass-throughs (as test_parity_at_size_gpu._count_deferred): one dict of counts per pass of FlowMatchingSampler._integrate
    (a graphed call makes two - the eager warm-up and the capture -, a replay none, an eager call one)."""
    KEYS = ("gemm_plain", "gemm_pair", "gemm_il", "gemm_norm", "gemm_rowsq", "gemm_row_scale", "attention", "attention_f16x3",
            "adarmsnorm", "rownorm_scale", "scratch")

    def __init__(self, monkeypatch):
        import covomix_amd.acoustic as ac
        import covomix_amd.ops as ops_
        self.passes = passes = []

        def count(key, n=1):
            if passes:
                passes[-1][key] += n

        def through(name, key):
            real = getattr(ops_, name)

            def fn(*a, **k):
                count(key)
                return real(*a, **k)
            monkeypatch.setattr(ops_, name, fn)
        real_gemm, real_integrate = ops_.gemm, ac.FlowMatchingSampler._integrate

        def gemm(a, w, out, **k):
            s = k.get("a_split")
            count("gemm_il" if isinstance(s, ops_.SplitIL) else "gemm_plain" if s is None else "gemm_pair")
            count("gemm_norm", k.get("norm") is not None)
            count("gemm_rowsq", k.get("c_rowsq") is not None)
            count("gemm_row_scale", k.get("a_row_scale") is not None)
            return real_gemm(a, w, out, **k)

        def integrate(self_, *a, **k):
            passes.append(dict.fromkeys(self.KEYS, 0))
            return real_integrate(self_, *a, **k)
        monkeypatch.setattr(ops_, "gemm", gemm)
        monkeypatch.setattr(ac.FlowMatchingSampler, "_integrate", integrate)
        for name, key in (("adarmsnorm", "adarmsnorm"), ("rownorm_scale", "rownorm_scale"), ("attention", "attention"),
                          ("attention_f16x3", "attention_f16x3"), ("_splitk_workspace", "scratch")):
            through(name, key)


def _quiet(fn, *a):
    """run a solve; a saturation re-run would put the call on the fp32 field - another route than the one the case names"""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn(*a)
    assert not any("saturat" in str(w.message) for w in rec), [str(w.message)[:100] for w in rec]
    return out


def _route_name(r):
    return "+".join(k for k in ("split_io", "interleaved", "fuse_norm", "splitk_scratch", "deferred", "graph") if getattr(r, k)) or "fp32-kernels"


@pytest.mark.parametrize("width,kind,case,precision", _equal_params())
def test_equal_length_route_and_accuracy(width, kind, case, precision, monkeypatch):
    import covomix_amd.ops as ops_
    B, T, s = case
    M = _rows(B, T, s)
    dims = MAIN if width == "main" else WIDE
    r = route(M, dims["dim"], precision)
    want = expected_record(r, dims["depth"], _comb_layers(_sd(width, kind)[0]), NFE)
    inp = _inputs(kind, B, T)
    model = _model(width, kind, precision)
    assert dataclasses.astuple(model._get_field().route(M)) == r          # the library's own record, field for field
    rec = _Recorder(monkeypatch)
    out = _quiet(_solve, model, inp, s)
    # 1. the route: a graphed shape makes the eager warm-up pass and the capture pass, an eager one a single pass - all on the same route
    assert len(rec.passes) == (2 if r.graph else 1), (len(rec.passes), r)
    for p in rec.passes:
        assert p == want, (r, p, want)
    ws = model._get_field()._ws[(B * (1 if s == 1.0 else 2), T)]
    assert isinstance(ws.get("normed16"), ops_.SplitIL) == r.interleaved
    # 4. the second call: a replay of the captured graph (no pass at all), the same bits
    again = _quiet(_solve, model, inp, s)
    assert len(rec.passes) == 2 and rec.passes[-1] == want          # (graphed: still the two of the first call; eager: one more)
    if r.graph:
        assert torch.equal(out, again)
    # 2. / 3. accuracy against fp64, and the figure
    ref64, ref32 = _reference(width, kind, inp, s, (B, T, s))
    e, e32 = rel_l2(out, ref64), rel_l2(ref32, ref64)
    worst = max(rel_l2(out[b], ref64[b]) for b in range(B))
    print(f"FIGURE acoustic-routes {width} dim={dims['dim']} {kind} {precision} B={B} T={T} scale={s} M={M} route={_route_name(r)} "
          f"err_vs_fp64={e:.3e} worst_utterance={worst:.3e} fp32_oracle_vs_fp64={e32:.3e} ratio={e / e32:.2f}")
    assert out.shape == (B, T, 80) and bool(torch.isfinite(out).all())
    tol = F16_ROLL_TOL if precision == "f16" else FP64_TOL
    assert e <= tol and worst <= 2 * tol, (e, worst)


FILL32, FILL16 = 1234.5, 1234.0          # recognisable, finite, exact in fp16


def _tails(v, M):
    """the rows behind M of a workspace entry: a tensor, a (hi, lo) pair, an interleaved pair or a list of those"""
    import covomix_amd.ops as ops_
    if isinstance(v, ops_.SplitIL):
        return [v.buf[M:]]
    if isinstance(v, (tuple, list)):
        return [t for x in v if x is not None for t in _tails(x, M)]
    return [v[M:]]


@pytest.mark.parametrize("kind,lengths,s", _ragged_params())
def test_ragged_route_accuracy_and_rows_behind_the_cut(kind, lengths, s, monkeypatch):
    import covomix_amd.ops as ops_
    per = isinstance(s, tuple)
    M = sum(lengths) * (2 if per or s != 1.0 else 1)
    r = route(M, MAIN["dim"], "f16x3", ragged_rows=M)
    want = expected_record(r, MAIN["depth"], _comb_layers(_sd("main", kind)[0]), NFE)
    utts = [_utt(kind, T) for T in lengths]
    model = _model("main", kind, "f16x3")
    field = model._get_field()
    assert dataclasses.astuple(field.route(M, ragged_rows=M)) == r        # the library's own record, field for field
    # 6. the capacity-sized workspace, made ahead of the solve (prepare() finds it under the same key): everything the kernels read or
    # write through the row views gets a recognisable value behind the cut
    full = field._workspace(0, 0, ragged_rows=M)
    assert full["xin"].shape[0] == r.ragged_capacity and (r.ragged_capacity - M) in range(0, 1024)
    filled = ("xin", "pred", "h", "normed16", "att16", "ff16", "pred16", "h16", "qk16")
    for k in filled:
        for t in _tails(full[k], M):
            t.fill_(FILL16 if t.dtype == torch.float16 else FILL32)
    rec = _Recorder(monkeypatch)
    outs = _quiet(_solve_ragged, model, utts, s)
    # 1. one eager pass on the route of the REAL row count, in the workspace of the capacity
    assert len(rec.passes) == 1 and rec.passes[0] == want, (r, rec.passes, want)
    assert field._ws.get(("ragged", r.ragged_capacity, M >= ops_.il_min_rows())) is full
    assert isinstance(full["normed16"], ops_.SplitIL) == r.interleaved
    # 2. / 3. every utterance against its own B = 1 fp64 run
    scales = s if per else (s,) * len(lengths)
    refs = [_utt_reference(kind, T, sc) for T, sc in zip(lengths, scales)]
    assert [tuple(o.shape) for o in outs] == [(T, 80) for T in lengths] and all(bool(torch.isfinite(o).all()) for o in outs)
    ref64, ref32, out = torch.cat([a for a, _ in refs]), torch.cat([b for _, b in refs]), torch.cat([o.cpu() for o in outs])
    e, e32 = rel_l2(out, ref64), rel_l2(ref32, ref64)
    worst = max(rel_l2(o, a) for o, (a, _) in zip(outs, refs))
    print(f"FIGURE acoustic-routes ragged dim={MAIN['dim']} {kind} f16x3 lengths={lengths} scale={s} M={M} capacity={r.ragged_capacity} "
          f"route={_route_name(r)} err_vs_fp64={e:.3e} worst_utterance={worst:.3e} fp32_oracle_vs_fp64={e32:.3e} ratio={e / e32:.2f}")
    assert e <= FP64_TOL and worst <= 2 * FP64_TOL, (e, worst)
    # 6. the buffers the kernels only write keep the fill behind the last row (xin, pred16, h16 and qk16 are filled so that a kernel
    # reading a row too far computes with a wrong value; they are written by the same kinds of store and not listed again.  vt16 is
    # left out: frames are its COLUMNS, and the zeros behind the last frame are read by the last key tile with weight 0.  None of the
    # listed buffers turned out to be written behind M by any route.)
    for k in ("pred", "h", "normed16", "att16", "ff16"):
        for t in _tails(full[k], M):
            assert bool((t == (FILL16 if t.dtype == torch.float16 else FILL32)).all()), (k, M, r.ragged_capacity)


REPLAY = dict(CROSSINGS)
REPLAY["64..129"] = CROSSINGS["64|65"] + CROSSINGS["127|128"]           # six workspace shapes through WORKSPACE_SHAPES = 4


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("crossing", list(REPLAY))
def test_one_model_runs_a_crossing_and_repeats_its_first_case(crossing, kind):
    """All cases of a crossing in order on ONE model object, then the first again: the same bits.  The 2048-row crossing holds five
    graphs (GRAPH_CACHE = 4: the first is evicted and captured again, in the workspace it had - two of its cases share the workspace of
    2 x 1024 rows), '64..129' six workspace shapes (the first is evicted, with the graph that kept it alive still cached)."""
    model = _model("main", kind, "f16x3")
    cases = REPLAY[crossing]
    outs = [_quiet(_solve, model, _inputs(kind, B, T), s) for B, T, s in cases]
    B, T, s = cases[0]
    assert torch.equal(_quiet(_solve, model, _inputs(kind, B, T), s), outs[0])
    assert all(bool(torch.isfinite(o).all()) for o in outs)


@pytest.mark.parametrize("group", [g for g in RAGGED if g != "r-per-utterance"])
def test_one_model_runs_a_ragged_crossing_and_repeats_its_first_case(group):
    """The same for ragged batches (eager launches): the smallest batch of a group runs again in the capacity workspace a larger one
    has used since (2046 rows after 2048 in the same 2048-row workspace; after 2050 took a 3072-row one)."""
    kind = KINDS[list(RAGGED).index(group) % 2]
    model = _model("main", kind, "f16x3")
    cases = RAGGED[group]
    outs = [_quiet(_solve_ragged, model, [_utt(kind, T) for T in lengths], s) for lengths, s in cases]
    lengths, s = cases[0]
    again = _quiet(_solve_ragged, model, [_utt(kind, T) for T in lengths], s)
    assert all(torch.equal(a, b) for a, b in zip(again, outs[0]))


def test_one_utterance_on_three_routes():
    """A fixed VoSingle utterance of 341 frames at scale 0.7 as the first of B = 3 (M = 2046: fused norms, K slices), the first of
    B = 4 (M = 2728: stand-alone norms, no scratch) and packed first in a ragged batch of 1024 frames (M = 2048: scratch without fused
    norms, per-row RoPE, per-sequence attention): the three results agree element by element within twice the fp64 bound times the
    largest |mel| of the utterance - a row that one route gets wrong shows here even where the rel-L2 of the whole batch hides it."""
    kind, T, s = "vosingle", 341, 0.7
    dim = MAIN["dim"]
    r3, r4, rr = route(2 * 3 * T, dim, "f16x3"), route(2 * 4 * T, dim, "f16x3"), route(2048, dim, "f16x3", ragged_rows=2048)
    assert (r3.fuse_norm, r3.splitk_scratch) == (True, True) and (r4.fuse_norm, r4.splitk_scratch) == (False, False)
    assert (rr.fuse_norm, rr.splitk_scratch, rr.ragged_capacity) == (False, True, 2048)
    u = _utt(kind, T)
    others = [{k: v[0] for k, v in _inputs(kind, 1, T).items()}] + [
        {k: v[j] for k, v in _inputs(kind, 3, T).items()} for j in range(2)]
    batch = lambda n: {k: torch.stack([u[k]] + [o[k] for o in others[:n - 1]]) for k in u}
    model = _model("main", kind, "f16x3")
    a = _quiet(_solve, model, batch(3), s)[0].cpu()
    b = _quiet(_solve, model, batch(4), s)[0].cpu()
    c = _quiet(_solve_ragged, model, [u, _utt(kind, 451), _utt(kind, 232)], s)[0].cpu()
    ref64, _ = _utt_reference(kind, T, s)
    bound = 2 * FP64_TOL * float(ref64.abs().max())
    diffs = {n: float((x.double() - y.double()).abs().max()) for n, x, y in (("B3-B4", a, b), ("B3-ragged", a, c), ("B4-ragged", b, c))}
    print(f"FIGURE acoustic-routes one-utterance T={T} max|a-b| {diffs} bound={bound:.3e} "
          f"err_vs_fp64 B3={rel_l2(a, ref64):.3e} B4={rel_l2(b, ref64):.3e} ragged={rel_l2(c, ref64):.3e}")
    assert all(rel_l2(x, ref64) <= 2 * FP64_TOL for x in (a, b, c))
    assert all(d <= bound for d in diffs.values()), (diffs, bound)
