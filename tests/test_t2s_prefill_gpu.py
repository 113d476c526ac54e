"""GPU: the text2semantic prefill pass - one causal full-sequence pass over tokens that are already known.

  1. cvx_t2s_prefill_attention_f32 alone against the fp64 oracle (both modes, one packed call), causality, the refused descriptors;
  2. score_many(prefill=True) against the fp64 oracle's teacher-forced logits: log-probs and raw logits, alone and among neighbours,
     twice, and beside the step chain;
  3. generate_many(prefixes=, prefill=True): the continuation against the oracle's choice, the log-probs, windows, the history rules;
  4. with the switch off, or on without a prefix, nothing moves (tokens, log-probs, graph cache keys, ABI version);
  5. the facade and the CLI flag.
The pass is fp32-class, NOT bit-identical to the step chain; it is bit-identical to itself, alone and among neighbours."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import t2s_geometry as geo
import t2s_logprob_restated as lrs
import t2s_oracle as orc
import t2s_prefill_restated as rs
from test_t2s_filters import load_small

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = 1.5
EINVAL = -22
SCORE_LEN, CONT_LEN = 272, 176
TARGET_LENS = (1, 33, 129, 257)


# ---------------------------------------------------------------- 1. the kernel alone
def _attend(d, causal, q=None, k=None, v=None):
    from covomix_amd import ops
    H = d["heads"]
    I = 64 * H
    cu = torch.tensor(d["cu"], dtype=torch.int32, device=DEV)
    q = (d["q"] if q is None else q).to(DEV)
    out = torch.full((q.shape[0], I), 7.0, device=DEV)
    max_q = max(rs.SEQ_LENS)
    if causal:                                   # the packed q | k | v buffer itself: kbase = cu
        qkv = torch.cat((q, (d["k"] if k is None else k).to(DEV), (d["v"] if v is None else v).to(DEV)), dim=1).contiguous()
        ops.t2s_prefill_attention(qkv[:, :I], qkv[:, I:2 * I], qkv[:, 2 * I:], out, cu, cu, None, max_q, H, rs.SCALE, True)
    else:                                        # k | v records, the rows behind every count NaN
        kv = d["kv"].to(DEV)
        kbase = torch.tensor(d["kbase_cross"], dtype=torch.int32, device=DEV)
        nk = torch.tensor(d["nk"], dtype=torch.int32, device=DEV)
        ops.t2s_prefill_attention(q.contiguous(), kv[:, :I], kv[:, I:], out, cu, kbase, nk, max_q, H, rs.SCALE, False)
    return out.cpu()


@pytest.mark.parametrize("heads", rs.HEADS)
@pytest.mark.parametrize("causal", [True, False])
def test_attention_against_fp64(heads, causal):
    d = rs.description(heads)
    k, v, kbase = (d["k"], d["v"], d["cu"][:-1]) if causal else (d["kv"][:, :64 * heads], d["kv"][:, 64 * heads:], d["kbase_cross"])
    ref = rs.oracle(d["q"], k, v, d["cu"], kbase, d["nk"], heads, causal)
    got = _attend(d, causal)
    err = rs.rel_l2(got, ref, d["cu"], heads)
    print(f"heads {heads}, causal {causal}: largest rel-L2 per (sequence, head) {float(err.max()):.3e} (bound {rs.REL_L2:.0e})")
    assert bool(torch.isfinite(got).all()), "a key row behind a count reached a result"
    assert float(err.max()) < rs.REL_L2, err
    assert torch.equal(_attend(d, causal), got), "the same call twice"


@pytest.mark.parametrize("heads", rs.HEADS)
def test_attention_is_causal(heads):
    """rows <= p of a sequence do not depend on its rows behind p, nor does any other sequence"""
    d = rs.description(heads)
    base = _attend(d, True)
    i, p = rs.SEQ_LENS.index(129), 40
    a, b = d["cu"][i] + p + 1, d["cu"][i + 1]
    g = torch.Generator().manual_seed(9)
    q, k, v = d["q"].clone(), d["k"].clone(), d["v"].clone()
    for t in (q, k, v):
        t[a:b] = torch.randn(b - a, t.shape[1], generator=g) * 3.0
    got = _attend(d, True, q, k, v)
    assert torch.equal(got[:a], base[:a]) and torch.equal(got[b:], base[b:])
    assert not torch.equal(got[a:b], base[a:b])


def test_attention_entry_refusals():
    """CVX_EINVAL and nothing launched: the output keeps its sentinel"""
    from covomix_amd import _lib, ops
    lib = _lib.load()
    H, I, M = 1, 64, 6
    qkv = torch.randn(M, 3 * I, device=DEV)
    cu = torch.tensor([0, 2, 6], dtype=torch.int32, device=DEV)
    out = torch.full((M, I), -7.0, device=DEV)
    size = C.sizeof(_lib.T2SPrefillAttention)

    def call(**edit):
        a = _lib.T2SPrefillAttention()
        a.struct_size, a.n, a.heads, a.causal, a.max_q, a.scale, a.rows = size, 2, H, 1, 4, rs.SCALE, M
        a.q, a.ldq, a.k, a.v, a.ldkv, a.out = qkv.data_ptr(), 3 * I, qkv.data_ptr() + 4 * I, qkv.data_ptr() + 8 * I, 3 * I, out.data_ptr()
        a.cu, a.kbase, a.nk = cu.data_ptr(), cu.data_ptr(), None
        for name, val in edit.items():
            setattr(a, name, val)
        rc = lib.cvx_t2s_prefill_attention_f32(C.byref(a), ops._stream())
        torch.cuda.synchronize()
        return rc

    for edit in (dict(struct_size=size - 8), dict(struct_size=size + 8), dict(struct_size=0), dict(n=0), dict(heads=0), dict(rows=-1),
                 dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(cu=None), dict(kbase=None), dict(causal=0, nk=None),
                 dict(max_q=0), dict(max_q=M + 1), dict(ldq=I - 4), dict(ldkv=3 * I + 2), dict(q=qkv.data_ptr() + 4)):
        assert call(**edit) == EINVAL, edit
    assert lib.cvx_t2s_prefill_attention_f32(None, ops._stream()) == EINVAL
    assert bool((out == -7.0).all())
    assert call(rows=0, max_q=0) == 0 and bool((out == -7.0).all())          # no rows: nothing to do
    assert call() == 0 and bool(torch.isfinite(out).all()) and not bool((out == -7.0).any())
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- 2. score_many(prefill=True) against the oracle
def _texts(src, n, seed):
    """n texts of different length cut from one text [1, T]"""
    gen = torch.Generator().manual_seed(seed)
    T = src.shape[1]
    out = []
    for _ in range(n):
        a = int(torch.randint(0, max(1, T // 2), (1,), generator=gen))
        e = int(torch.randint(a + 3, T + 1, (1,), generator=gen))
        out.append(src[:, a:e])
    return out


def _targets(S, V, lengths, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(0, V - 1, (S, L), generator=gen) for L in lengths]


_CASES = {}


def _case(name):
    """(state dict, decoder with max_length SCORE_LEN, texts, targets, fp64 teacher-forced logits per utterance) - built once"""
    from covomix_amd.t2s import TextToSemanticDecoder
    if name in _CASES:
        return _CASES[name]
    scale = CFG if name.endswith("+cfg") else 1.0
    base = name.split("+")[0]
    if base in geo.CASES:
        sd = geo.state_dict(base)
        model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=SCORE_LEN, max_source=geo.MAX_SOURCE)
        srcs = [geo.text(n, seed=30 + n) for n in (3, 15, 7, 11)]
    else:
        g, sd = load_small(base)
        model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=SCORE_LEN)
        srcs = _texts(torch.from_numpy(g["source_ids"]), len(TARGET_LENS), seed=41)
    tg = _targets(model.d["streams"], model.d["vocab"], TARGET_LENS, seed=43)
    lg64 = [orc.teacher_forced_logits(sd, s_, t_, cond_scale=scale, dtype=torch.float64) for s_, t_ in zip(srcs, tg)]
    _CASES[name] = (sd, model, srcs, tg, lg64, scale)
    return _CASES[name]


def _bound_ratio(lg64, streams, lp):
    """largest |lp - lp64| / bound over the positions, with the bound of tests/test_t2s_logprobs_gpu.py::_oracle_check:
    2 LONG_LOGIT_TOL ||logits64[pos, s]||_2 + 256 * 2^-24 (1 + |lp64|)"""
    lp64 = torch.log_softmax(lg64, dim=-1).gather(-1, streams.T[..., None])[..., 0].T                        # [S, L]
    bound = 2 * orc.LONG_LOGIT_TOL * lg64.norm(dim=-1).T + lrs.bound(lp64)
    assert lp.shape == streams.shape and lp.dtype == torch.float32
    return float(((lp.double().cpu() - lp64).abs() / bound).max())


SCORE_CASES = ["cosingle_small", "comix_small", "cosingle_small+cfg", "k260-h3-v501", "two-k520-v333"]


@pytest.mark.parametrize("name", SCORE_CASES)
def test_prefill_scores_against_the_oracle(name):
    from covomix_amd import ops
    sd, model, srcs, tg, lg64, scale = _case(name)
    keys = set(model._graphs)
    lps, lgs = model._score_prefill(srcs, tg, [scale] * len(tg), return_logits=True)
    assert set(model._graphs) == keys, "a pass takes no graph"
    pub = model.score_many(srcs, tg, cond_scale=scale, prefill=True)
    worst = 0.0
    for j, L in enumerate(TARGET_LENS):
        assert torch.equal(pub[j], lps[j]), "the same call twice"
        assert pub[j].device.type == "cpu" and tuple(pub[j].shape) == (model.d["streams"], L)
        pos = orc.per_position_rel_l2(lgs[j], lg64[j])
        ratio = _bound_ratio(lg64[j], tg[j], lps[j])
        worst = max(worst, ratio)
        print(f"{name} L = {L}: logits rel-L2 per position, largest {float(pos.max()):.3e} (bound {orc.LONG_LOGIT_TOL:.1e}); "
              f"log-prob error / bound {ratio:.3f}")
        assert float(pos.max()) <= orc.LONG_LOGIT_TOL, (name, L)
        assert ratio <= 1.0, (name, L, ratio)
    print(f"{name}: largest log-prob error / bound {worst:.3f}")
    # alone == among the others, bit for bit: every form the fp32 GEMM picks by M accumulates an output element in the same order
    # (DESIGN.md 4.6), and attention, norm and GEGLU work row by row / sequence by sequence
    for j in range(len(tg)):
        alone = model.score_many([srcs[j]], [tg[j]], cond_scale=scale, prefill=True)[0]
        assert _bound_ratio(lg64[j], tg[j], alone) <= 1.0
        assert torch.equal(alone, lps[j]), (name, j)
    # beside the step chain: both inside the bound, not equal by contract
    steps = model.score_many(srcs, tg, cond_scale=scale)
    diff = max(float((a - b).abs().max()) for a, b in zip(steps, lps))
    print(f"{name}: largest |pass - step chain| log-prob difference {diff:.3e}")
    for j in range(len(tg)):
        assert _bound_ratio(lg64[j], tg[j], steps[j]) <= 1.0, (name, "step chain", j)


def test_prefill_scores_mixed_guidance_in_one_pass():
    sd, model, srcs, tg, lg64, _ = _case("cosingle_small")
    _, _, _, _, lg64g, _ = _case("cosingle_small+cfg")
    scales = [1.0, CFG, CFG, 1.0]
    got = model.score_many(srcs, tg, cond_scale=scales, mixed_guidance=True, prefill=True)
    for j, c in enumerate(scales):
        assert _bound_ratio((lg64g if c > 1 else lg64)[j], tg[j], got[j]) <= 1.0, j
        assert torch.equal(got[j], model.score_many([srcs[j]], [tg[j]], cond_scale=c, prefill=True)[0]), j
    with pytest.raises(NotImplementedError):
        _case("comix_small")[1].score_many(srcs[:1], [_case("comix_small")[3][0]], cond_scale=CFG, prefill=True)


# ---------------------------------------------------------------- 3. continuation
_CONT = {}


def _cont_model(name):
    from covomix_amd.t2s import TextToSemanticDecoder
    if name not in _CONT:
        g, sd = load_small(name)
        _CONT[name] = (g, sd, TextToSemanticDecoder(sd, torch.device(DEV), max_length=CONT_LEN))
    return _CONT[name]


def _uniforms(n, steps, S, V, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand(steps, S, V, generator=gen).clamp_(1e-6, 1 - 1e-6) for _ in range(n)]


def _decidable(sd, src, streams, uni, P, scale=1.0):
    """(fp64 logits of the returned tokens, the reference's tokens [steps, S] from position P on, decidable [steps, S])"""
    lg64 = orc.teacher_forced_logits(sd, src, streams, cond_scale=scale, dtype=torch.float64)
    L = streams.shape[1]
    tok, ok = orc.reference_choice(lg64[P:L], uni[P:L])
    return lg64, tok, ok


@pytest.mark.parametrize("name,scale", [("cosingle_small", 1.0), ("comix_small", 1.0), ("cosingle_small", CFG)])
def test_continuation_from_a_prefilled_prefix(name, scale):
    g, sd, model = _cont_model(name)
    S, V = model.d["streams"], model.d["vocab"]
    STEPS, PS = 31, (129, 1, 33)
    srcs = _texts(torch.from_numpy(g["source_ids"]), 3, seed=51)
    pre = _targets(S, V, PS, seed=1)
    unis = _uniforms(3, max(PS) + STEPS, S, V, seed=2)
    limits = [P + STEPS for P in PS]
    armed = []
    real = model._prefill_slots
    model._prefill_slots = lambda *a: (real(*a), armed.append(a[5].clone()))[0]
    try:
        res = model.generate_many(srcs, unis, limits=limits, ignore_eos=True, cond_scale=scale, prefixes=pre, prefill=True, return_logprobs=True)
    finally:
        del model._prefill_slots
    slots_per = 2 if scale > 1.0 else 1
    assert len(armed) == 1 and [int(armed[0][slots_per * j + h, 0]) for j in range(3) for h in range(slots_per)] == \
        [P for P in PS for _ in range(slots_per)], "the slot records start at P"
    assert [rec[4] for rec in model.last_records] == limits
    n_ok = n_all = 0
    for j, P in enumerate(PS):
        flat, streams, lp = res[j]
        assert tuple(streams.shape) == (S, P + STEPS) and torch.equal(streams[:, :P], pre[j]), "streams starts with the prefix"
        lg64, tok, ok = _decidable(sd, srcs[j], streams, unis[j], P, scale)
        assert bool((tok[ok] == streams[:, P:].T[ok]).all()), (name, j, "a decidable step disagrees with the reference's choice")
        n_ok, n_all = n_ok + int(ok.sum()), n_all + ok.numel()
        below, behind = _bound_ratio(lg64[:P], streams[:, :P], lp[:, :P]), _bound_ratio(lg64[P:], streams[:, P:], lp[:, P:])
        print(f"{name} scale {scale} P = {P}: log-prob error / bound {below:.3f} below P, {behind:.3f} from P on")
        assert below <= 1.0 and behind <= 1.0
    print(f"{name} scale {scale}: {n_ok} of {n_all} sampled steps decidable")
    assert n_ok >= 0.9 * n_all
    # the prefix positions are the pass' own log-probs; the step chain's continuation equals the chain's without prefill where it is decidable
    scored = model.score_many(srcs, pre, cond_scale=scale, prefill=True)
    for j, P in enumerate(PS):
        assert torch.equal(res[j][2][:, :P], scored[j]), j


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_windows_and_history_rules(name):
    """5 prefixed utterances through 2 slots (windows of 2): every utterance gets the tokens it gets alone; no 2-gram repeats across prefix
    and continuation under no_repeat_ngram_size = 2"""
    g, sd, model = _cont_model(name)
    S, V = model.d["streams"], model.d["vocab"]
    STEPS, PS = 15, (5, 17, 33, 40, 64)
    srcs = _texts(torch.from_numpy(g["source_ids"]), 5, seed=61)
    pre = _targets(S, V, PS, seed=3)
    pre[2] = None                                                     # one utterance of the call has no prefix
    unis = _uniforms(5, max(PS) + STEPS, S, V, seed=4)
    limits = [P + STEPS for P in PS]
    kw = dict(ignore_eos=True, prefill=True, return_logprobs=True)
    many = model.generate_many(srcs, unis, limits=limits, slots=2, prefixes=pre, **kw)
    for j in range(5):
        alone = model.generate_many(srcs[j:j + 1], unis[j:j + 1], limits=limits[j:j + 1], prefixes=pre[j:j + 1], **kw)[0]
        if not torch.equal(alone[1], many[j][1]):                     # (allowed only where a step of either run is undecidable)
            P = 0 if pre[j] is None else PS[j]
            oks = [_decidable(sd, srcs[j], r[1], unis[j], P)[2] for r in (alone, many[j])]
            assert not all(bool(o.all()) for o in oks), (name, j)
        else:
            assert torch.equal(alone[2], many[j][2]), (name, j)
    ruled = model.generate_many(srcs, unis, limits=limits, slots=2, prefixes=pre, no_repeat_ngram_size=2, **kw)
    for j, r in enumerate(ruled):
        P = 0 if pre[j] is None else PS[j]
        for s in range(S):
            row = r[1][s].tolist()
            seen = set(zip(row[:max(P - 1, 0)], row[1:P]))
            for t in range(max(P, 1), len(row)):
                assert (row[t - 1], row[t]) not in seen, (name, j, s, t)
                seen.add((row[t - 1], row[t]))


# ---------------------------------------------------------------- 4. off means off
@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_nothing_moves_when_prefill_is_off_or_has_no_prefix(name):
    from covomix_amd import _lib
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_small(name)
    model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=40)
    S, V = model.d["streams"], model.d["vocab"]
    src = torch.from_numpy(g["source_ids"])
    uni = torch.from_numpy(g["uniforms"])[:40, :, 0, :]
    gold = torch.from_numpy(g["streams"])[0, :, :40]
    srcs, unis = [src, src[:, :5]], [uni, uni.flip(0).contiguous()]
    base = model.generate_many(srcs, unis, slots=2, return_logprobs=True)
    assert torch.equal(base[0][1], gold[:, :base[0][1].shape[1]]), "the tokens of the golden decode"
    keys = set(model._graphs)
    for kw in (dict(prefill=False), dict(prefill=True), dict(prefill=True, prefixes=[None, None])):
        got = model.generate_many(srcs, unis, slots=2, return_logprobs=True, **kw)
        if "prefixes" not in kw:
            assert set(model._graphs) == keys, kw
        for a, b in zip(base, got):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), kw
    pre = [base[0][1][:, :3], None]
    plain = model.generate_many(srcs, unis, slots=2, return_logprobs=True, prefixes=pre)
    keys = set(model._graphs)
    off = model.generate_many(srcs, unis, slots=2, return_logprobs=True, prefixes=pre, prefill=False)
    assert set(model._graphs) == keys and all(torch.equal(x, y) for a, b in zip(plain, off) for x, y in zip(a, b))
    tg = [r[1] for r in base]
    scored = model.score_many(srcs, tg)
    keys = set(model._graphs)
    assert all(torch.equal(a, b) for a, b in zip(scored, model.score_many(srcs, tg, prefill=False))) and set(model._graphs) == keys
    assert all(torch.equal(a, r[2]) for a, r in zip(scored, base)), "the step chain's scores are the sampled log-probs, as ever"
    model.score_many(srcs, tg, prefill=True)
    assert set(model._graphs) == keys
    assert _lib.load().cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- 5. facade and CLI
def test_facade_scoring_and_prefix():
    from covomix_amd.conditional_model import CoVoMixModel
    g, sd = load_small("cosingle_small")
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval().to(DEV)
    dec = m._get_t2s()
    ids = [t.to(DEV) for t in _texts(torch.from_numpy(g["source_ids"]), 2, seed=7)]
    tg = _targets(1, dec.d["vocab"], (9, 30), seed=8)
    for scale in (1.0, CFG):
        want = dec.score_many(ids, tg, cond_scale=scale, prefill=True)
        got = m.score_text2semantic(ids, tg, cond_scale=scale, prefill=True)
        assert all(torch.equal(a, b) for a, b in zip(want, got))
        assert torch.equal(m.score_text2semantic(ids[1], tg[1], cond_scale=scale, prefill=True), want[1])
    uni = _uniforms(1, 24, 1, dec.d["vocab"], seed=9)[0]
    a = m.synthesis_sample_text2semantic(ids[0], uniforms=uni, max_length=24, prefix=tg[0], prefill=True, return_logprobs=True)
    b = dec.generate_many([ids[0]], [uni], 24, prefixes=[tg[0]], prefill=True, return_logprobs=True)[0]
    assert torch.equal(a[1].cpu(), b[1]) and torch.equal(a[2].cpu(), b[2]) and torch.equal(a[1][:, :9].cpu(), tg[0])
    with pytest.raises(ValueError, match="mixed_guidance"):
        m.synthesis_sample_text2semantic([ids[0]], uniforms=[uni], max_length=24, prefix=[tg[0]], prefill=True, mixed_guidance=True)


def test_cli_prefill(tmp_path, monkeypatch):
    """a two-turn dialogue whose first turn has a .prefix.semantic.npy: --t2s_prefill runs, hands the switch and the prefix to the facade
    and writes the files of the run without it"""
    import covomix_amd.synthetic as syn
    from covomix_amd import generation
    from test_generation_gpu import _write_fixture
    tmp = str(tmp_path)
    _write_fixture(tmp, "vosingle")
    shapes = syn.t2s_param_shapes(two_output=False, dim=64, dim_target=64, source_depth=2, target_depth=2, heads=1, num_text=200)
    tsd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=0).items()}
    torch.save({"state_dict": {"cfm_wrapper.model." + k: v for k, v in tsd.items()},
                "hyper_parameters": {"text2semantic": True}}, os.path.join(tmp, "t2s.ckpt"))
    tdir, pdir = os.path.join(tmp, "text"), os.path.join(tmp, "prompt")
    os.makedirs(tdir); os.makedirs(pdir)
    rng = np.random.RandomState(1)
    for suf in ("_1", "_2"):
        np.save(os.path.join(pdir, f"dlg_a{suf}.hubert_code.npy"), rng.randint(0, 500, size=20))
        np.save(os.path.join(pdir, f"dlg_a{suf}.mel.npy"), (rng.randn(80, 20) * 2 - 6).astype(np.float32))
    for k in range(2):
        np.save(os.path.join(tdir, f"dlg_a.turn{k}.text_ids.npy"), rng.randint(1, 199, size=(1, 7 + k)).astype(np.int64))
    prefix = rng.randint(0, 100, size=5).astype(np.int64)
    np.save(os.path.join(tdir, "dlg_a.turn0.prefix.semantic.npy"), prefix)
    real = generation.CoVoMixModel.synthesis_sample_text2semantic
    seen = []

    def spy(self, ids, **kw):
        out = real(self, ids, max_length=12, **kw)
        seen.append((kw.get("prefill", False), kw.get("prefix"), [t.cpu() for t in out]))
        return out
    monkeypatch.setattr(generation.CoVoMixModel, "synthesis_sample_text2semantic", spy)
    base = ["--t2s_ckpt", os.path.join(tmp, "t2s.ckpt"), "--acous_ckpt", os.path.join(tmp, "acous.ckpt"),
            "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"), "--text_dir", tdir, "--prompt_dir", pdir, "--mode", "covosingle"]
    with pytest.warns(UserWarning, match="EMA"):
        for out, extra in (("o0", []), ("o1", ["--t2s_prefill"])):
            assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, out)] + extra) == 1
    assert sorted(os.listdir(os.path.join(tmp, "o0"))) == sorted(os.listdir(os.path.join(tmp, "o1")))
    assert [s_[0] for s_ in seen] == [False, True] and all(s_[1] is not None and s_[1][0] is not None for s_ in seen)
    for s_ in seen:
        assert s_[2][0][:5].tolist() == prefix.tolist(), "the first turn starts with its prefix"
