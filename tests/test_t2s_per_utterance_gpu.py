"""GPU: per-utterance sampling settings and forced prefixes of the text2semantic decode (cvx_t2s_decode_steps_per_dialogue,
generate_many(settings=, prefixes=), the facade's list-valued arguments, the CLI's side files).  Every comparison is EXACT: an
utterance gets, bit for bit, the tokens and log-probs it gets alone on the scalar path with its own settings."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_t2s_filters import DECODE_STEPS, decode_uniforms, load_small
from test_t2s_filters_gpu import _texts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
NAMES = ["cosingle_small", "comix_small"]
N_MIXED = 12


def _settings(V):
    """the six settings of the mixed queue; [0] is the default"""
    return [dict(temperature=1.0),
            dict(temperature=0.7, filter_logits_fn="top_k", filter_fn_kwargs={"k": 7}),
            dict(temperature=1.3, filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.9}),
            dict(temperature=1.0, filter_logits_fn="top_k", filter_fn_kwargs={"k": 1}),
            dict(temperature=0, filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.5}),
            dict(temperature=1.0, filter_logits_fn="top_k", filter_fn_kwargs={"k": V})]


class Case:
    """one small model, the 12 texts with their own draws, and every (utterance, setting) decoded ALONE on the scalar path - once"""

    def __init__(self, name):
        from covomix_amd.t2s import TextToSemanticDecoder
        self.name = name
        self.g, sd = load_small(name)
        self.model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=256)
        self.S, self.V = self.g["uniforms"].shape[1], self.g["uniforms"].shape[-1]
        self.srcs = _texts(self.g, N_MIXED, seed=11)
        self.unis = [decode_uniforms(self.S, self.V, salt=300 + i) for i in range(N_MIXED)]
        self.sets = _settings(self.V)
        self._alone = {}

    def alone(self, j, si):
        """(flat, streams, logprobs) of utterance j alone with setting si, host tensors"""
        if (j, si) not in self._alone:
            r = self.model.generate(self.srcs[j], uniforms=self.unis[j], return_logprobs=True, **self.sets[si])
            self._alone[(j, si)] = tuple(t.cpu() for t in r)
        return self._alone[(j, si)]

    def warm(self, pairs):
        for si in sorted({si for _, si in pairs}):               # (setting by setting: one captured graph at a time)
            for j in [j for j, s_ in pairs if s_ == si]:
                self.alone(j, si)


@pytest.fixture(scope="module")
def cases():
    return {n: Case(n) for n in NAMES}


def _same(res, want):
    return all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(res, want)) and len(res) == len(want) == 3


# ---------------------------------------------------------------- 1. mixed settings == alone
@pytest.mark.parametrize("slots", [1, 8, 16])
@pytest.mark.parametrize("name", NAMES)
def test_mixed_settings_equal_alone(cases, name, slots):
    """12 utterances, six settings in turn, through 1 / 8 / 16 slots (8: refills carry the settings into a slot that held another
    dialogue; 16: two kernel groups): every utterance == its decode alone with its settings as the call's scalars - tokens, streams and
    log-probs.  At 8 slots once more with the settings rotated by one against the texts (a table indexed by the slot would survive the
    first run), and every non-default setting changes at least one of its utterances."""
    c = cases[name]
    for rot in ((0, 1) if slots == 8 else (0,)):
        pick = [(j + rot) % len(c.sets) for j in range(N_MIXED)]
        c.warm([(j, pick[j]) for j in range(N_MIXED)])
        res = c.model.generate_many(c.srcs, c.unis, slots=slots, return_logprobs=True, settings=[c.sets[si] for si in pick])
        rec = c.model.last_records
        for j in range(N_MIXED):
            assert _same(res[j], c.alone(j, pick[j])), (name, slots, rot, j, pick[j], rec[j])
        if slots == 8:
            assert len({rec[j][5] for j in range(N_MIXED)}) == 8
        if slots == 8 and rot == 0:
            c.warm([(j, 0) for j in range(N_MIXED)])
            for si in range(1, len(c.sets)):
                mine = [j for j in range(N_MIXED) if pick[j] == si]
                assert any(not torch.equal(c.alone(j, si)[1], c.alone(j, 0)[1]) for j in mine), (name, "setting", si, "did not arrive")
    # entries that leave fields out take the call's scalars
    if slots == 8:
        part = c.model.generate_many(c.srcs[:3], c.unis[:3], slots=2, temperature=0.7, filter_logits_fn="top_k", filter_fn_kwargs={"k": 7},
                                     return_logprobs=True, settings=[None, c.sets[2], {"temperature": 0.7}])
        assert _same(part[0], c.alone(0, 1)) and _same(part[1], c.alone(1, 2)) and _same(part[2], c.alone(2, 1))


# ---------------------------------------------------------------- 2. the reference's tokens inside a mixed queue
@pytest.mark.parametrize("name", NAMES)
def test_reference_pin_inside_a_mixed_queue(cases, name):
    c = cases[name]
    gold = torch.from_numpy(c.g["uniforms"])[:, :, 0, :]
    srcs, unis = list(c.srcs[:8]), list(c.unis[:8])
    sets = [c.sets[1 + j % 5] for j in range(8)]
    srcs[5], sets[5] = torch.from_numpy(c.g["source_ids"]), None
    unis[5] = torch.cat((gold, unis[5][gold.shape[0]:]))
    limits = [DECODE_STEPS] * 8
    limits[5] = gold.shape[0]
    res = c.model.generate_many(srcs, unis, slots=4, limits=limits, settings=sets)
    assert torch.equal(res[5][0], torch.from_numpy(c.g["tokens"])), name
    for j in (0, 7):
        assert torch.equal(res[j][1], c.alone(j, 1 + j % 5)[1])


def test_guided_scales_inside_one_queue(cases):
    """the guided fixture's text at its own scale among guided utterances at 2.0 and 3.0, four slot pairs: the reference's tokens for
    it, and every utterance == its guided decode alone at ITS scale"""
    c = cases["cosingle_small"]
    gold = np.load(os.path.join(GOLDEN, "t2s_cosingle_small_cfg.npz"))
    scale = float(gold["cond_scale"])
    gu = torch.from_numpy(gold["uniforms"])[:, :, 0, :]
    n, at = 7, 3
    srcs, unis = list(c.srcs[:n]), list(c.unis[:n])
    scales = [2.0 if j % 2 else 3.0 for j in range(n)]
    srcs[at], unis[at], scales[at] = torch.from_numpy(gold["source_ids"]), torch.cat((gu, unis[at][gu.shape[0]:])), scale
    limits = [DECODE_STEPS] * n
    limits[at] = gu.shape[0]
    sets = [None if j == at else {"cond_scale": scales[j]} for j in range(n)]
    sets[1] = dict(sets[1], temperature=0.7, filter_logits_fn="top_p")
    res = c.model.generate_many(srcs, unis, slots=8, limits=limits, cond_scale=scale, return_logprobs=True, settings=sets)
    assert torch.equal(res[at][0], torch.from_numpy(gold["tokens"]))
    for j in range(n):
        kw = dict(temperature=0.7, filter_logits_fn="top_p") if j == 1 else {}
        alone = c.model.generate(srcs[j], uniforms=unis[j][:limits[j]], cond_scale=scales[j], return_logprobs=True, **kw)
        assert _same(res[j], tuple(t.cpu() for t in alone)), (j, scales[j])
    assert not torch.equal(res[0][1], c.model.generate(srcs[0], uniforms=unis[0], cond_scale=2.0, return_streams=True)[1].cpu())
    with pytest.raises(ValueError, match="two calls"):
        c.model.generate_many(srcs[:2], unis[:2], cond_scale=scale, settings=[None, {"cond_scale": 1.0}])
    with pytest.raises(ValueError, match="two calls"):
        c.model.generate_many(srcs[:2], unis[:2], settings=[None, {"cond_scale": 2.0}])


# ---------------------------------------------------------------- 3. / 4. resume identity
N_RESUME = 10


@pytest.fixture(scope="module")
def resumed(cases):
    """run A per model: 10 utterances sampled under ignore_eos with limits around 40 steps, and the prefix lengths of run B - from
    {1, 15, 16, 17, limit - 1}, either side of the 16-step chunk, cut below the first eos where A sampled one"""
    out = {}
    for name in NAMES:
        c = cases[name]
        srcs, unis = c.srcs[:N_RESUME], c.unis[:N_RESUME]
        limits = [40 + j % 4 for j in range(N_RESUME)]
        sets = [c.sets[j % 3] for j in range(N_RESUME)]
        A = c.model.generate_many(srcs, unis, slots=8, ignore_eos=True, limits=limits, return_logprobs=True, settings=sets)
        P = []
        for j in range(N_RESUME):
            want = [1, 15, 16, 17, limits[j] - 1][j % 5]
            hit = (A[j][1] == c.V - 1).any(dim=0).nonzero()
            P.append(min(want, int(hit[0])) if hit.numel() else want)
        assert all(p >= 1 for p in P), (name, P)
        assert tuple(A[0][1].shape) == (c.S, limits[0])
        out[name] = dict(srcs=srcs, unis=unis, limits=limits, sets=sets, A=A, P=P, prefixes=[A[j][1][:, :P[j]] for j in range(N_RESUME)])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_resume_identity(cases, resumed, name):
    """B continues from A's first P tokens with A's draws: A's streams and log-probs over the whole length; the prefix positions hold
    what score_many gives those tokens"""
    c, r = cases[name], resumed[name]
    B = c.model.generate_many(r["srcs"], r["unis"], slots=8, ignore_eos=True, limits=r["limits"], return_logprobs=True, settings=r["sets"],
                              prefixes=r["prefixes"])
    print(name, "prefix lengths", r["P"])
    for j in range(N_RESUME):
        assert _same(B[j], r["A"][j]), (name, j, r["P"][j])
    scored = c.model.score_many(r["srcs"], r["prefixes"])
    for j in range(N_RESUME):
        assert torch.equal(scored[j], B[j][2][:, :r["P"][j]]), (name, j)
    # prefixes alone (no settings), some utterances without one, through the pinned result path of a refilled queue
    some = [p if j % 2 else None for j, p in enumerate(r["prefixes"])]
    D = c.model.generate_many(r["srcs"], r["unis"], slots=4, ignore_eos=True, limits=r["limits"], return_logprobs=True, prefixes=some)
    for j in range(N_RESUME):
        if r["sets"][j] is c.sets[0]:
            assert _same(D[j], r["A"][j]), (name, j)
    with pytest.raises(ValueError, match="eos"):
        c.model.generate_many(r["srcs"][:1], r["unis"][:1], prefixes=[torch.full((c.S, 2), c.V - 1)])
    with pytest.raises(ValueError, match="forced"):
        c.model.generate_many(r["srcs"][:1], [None], return_logprobs=True, forced=[r["prefixes"][0]], prefixes=[r["prefixes"][0]])


@pytest.mark.parametrize("name", NAMES)
def test_prefix_without_scoring(cases, resumed, name):
    """the forced read of the instantiation WITHOUT the log-prob epilogue: the same tokens"""
    c, r = cases[name], resumed[name]
    B = c.model.generate_many(r["srcs"], r["unis"], slots=8, ignore_eos=True, limits=r["limits"], settings=r["sets"], prefixes=r["prefixes"])
    for j in range(N_RESUME):
        assert len(B[j]) == 2 and torch.equal(B[j][0], r["A"][j][0]) and torch.equal(B[j][1], r["A"][j][1]), (name, j, r["P"][j])


# ---------------------------------------------------------------- 5. / 6. the entry point itself
def _per_struct(model, n_records=None, size=None, table=True):
    from covomix_amd import _lib
    t = model.buf["per"]
    return _lib.T2SPerDialogue(C.sizeof(_lib.T2SPerDialogue) if size is None else size, t.shape[0] if n_records is None else n_records,
                               t.data_ptr() if table else None)


def test_no_queue_slot_b_is_dialogue_b(cases):
    """cvx_t2s_decode_steps_per_dialogue without a queue: four slots, four rows of settings, the tokens of the four decodes alone"""
    from covomix_amd import _lib, ops
    from covomix_amd.t2s import check_settings, settings_rows
    c = cases["comix_small"]
    m, nb, steps = c.model, 4, DECODE_STEPS
    pick = [1, 2, 4, 0]
    c.warm([(b, pick[b]) for b in range(nb)])
    m._ensure(nb, nb, steps)
    ctx = m._contexts(c.srcs[:nb])
    for b in range(nb):
        m._uniform_view(nb)[b, :steps].copy_(c.unis[b].to(DEV))
    m.buf["tokens"].zero_()
    m.buf["per"].zero_()
    m.buf["per"][:nb].copy_(settings_rows(check_settings([c.sets[si] for si in pick], nb, c.V, c.S)).to(DEV))
    m.buf["x"][:nb].copy_(m.start[None, :].expand(nb, -1))
    m.buf["state"].copy_(m._slot_records(ctx))
    dec = m._descriptor(-1.0, nb)                          # (the descriptor's own scalars are ignored: they need not be valid)
    dec.filter_mode, dec.top_k, dec.top_p = 9, 0, 7.0
    per = _per_struct(m)
    rc = _lib.load().cvx_t2s_decode_steps_per_dialogue(C.byref(dec), None, C.byref(per), steps, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    for b in range(nb):
        want = c.alone(b, pick[b])[1]
        assert torch.equal(m.buf["tokens"][b, :, :want.shape[1]].cpu(), want), (b, pick[b])


def test_refusals_launch_nothing(cases):
    from covomix_amd import _lib, ops
    c = cases["cosingle_small"]
    m, lib = c.model, _lib.load()
    m._ensure(8, 8, 16, True)
    sentinel = torch.full_like(m.buf["state"], 5)          # position 5: a launch would advance it and write a token
    m.buf["state"].copy_(sentinel)
    m.buf["tokens"].fill_(3)
    size = C.sizeof(_lib.T2SPerDialogue)
    sc = _lib.T2SScoring(C.sizeof(_lib.T2SScoring), m.max_length, m.buf["logprobs"].data_ptr())

    def call(per, scoring=None, null_per=False, **edit):
        dec = m._descriptor(1.0, edit.pop("batch", 8), edit.pop("cfg_scale", 1.0), edit.pop("queue", False), None, edit.pop("nd", 0))
        for k, v in edit.items():
            setattr(dec, k, v)
        rc = lib.cvx_t2s_decode_steps_per_dialogue(C.byref(dec), None if scoring is None else C.byref(scoring), None if null_per else C.byref(per),
                                                   1, ops._stream())
        torch.cuda.synchronize()
        return rc

    assert call(_per_struct(m, size=size - 4)) == EINVAL and call(_per_struct(m, size=size + 8)) == EINVAL and call(_per_struct(m, size=0)) == EINVAL
    assert call(_per_struct(m, table=False)) == EINVAL                      # NULL table
    assert call(None, null_per=True) == EINVAL
    assert call(_per_struct(m, n_records=0)) == EINVAL
    assert call(_per_struct(m, n_records=7), queue=True, nd=8) == EINVAL    # fewer rows than dialogue records
    assert call(_per_struct(m, n_records=7)) == EINVAL                      # ... than slots, without a queue
    assert call(_per_struct(m), scoring=_lib.T2SScoring(8, m.max_length, m.buf["logprobs"].data_ptr())) == EINVAL
    assert call(_per_struct(m), scoring=_lib.T2SScoring(16, m.max_length, None)) == EINVAL
    assert call(_per_struct(m), batch=65) == EINVAL and call(_per_struct(m), state=None) == EINVAL
    assert call(_per_struct(m), cfg_scale=2.0, queue=True, nd=7) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(m.buf["state"], sentinel) and bool((m.buf["tokens"] == 3).all())
    # the ignored scalars are no reason to refuse: idle slots (position max_length), so this launch writes nothing either
    m.buf["state"].copy_(m._slot_records([]))
    assert call(_per_struct(m), scoring=sc, temperature=-1.0, filter_mode=5, top_k=0, top_p=2.0) == 0
    assert bool((m.buf["tokens"] == 3).all())
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION


# ---------------------------------------------------------------- 7. the old paths
def test_old_paths_untouched(cases):
    c = cases["cosingle_small"]
    m = c.model
    is_per = lambda k: k[0] == "per"
    m._graphs.clear()
    a = m.generate_many(c.srcs[:3], c.unis[:3], slots=2, settings=None, prefixes=None)
    b = m.generate_many(c.srcs[:3], c.unis[:3], slots=2)
    assert not any(is_per(k) for k in m._graphs) and len(m._graphs) == 1
    for x, y in zip(a, b):
        assert torch.equal(x[1], y[1])
    # one "per" graph serves every mix of settings
    m.generate_many(c.srcs[:3], c.unis[:3], slots=2, settings=[c.sets[1], c.sets[2], None])
    m.generate_many(c.srcs[:3], c.unis[:3], slots=2, settings=[c.sets[4], None, c.sets[5]], temperature=0.3)
    m.generate_many(c.srcs[:3], c.unis[:3], slots=2, prefixes=[None, a[1][1][:, :1], None])
    assert sum(1 for k in m._graphs if is_per(k)) == 1 and len(m._graphs) == 2


# ---------------------------------------------------------------- 8. facade
@pytest.mark.parametrize("name", NAMES)
def test_facade_lists_and_best_of_temperatures(cases, name):
    from covomix_amd.conditional_model import CoVoMixModel
    from covomix_amd.t2s import best_candidate, sequence_logprob
    c = cases[name]
    g, sd = load_small(name)
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval().to(DEV)
    S, V, steps = c.S, c.V, 24
    ids, us = c.srcs[:3], [u[:steps] for u in c.unis[:3]]
    temps, fns, kws = [0.7, 1.0, 1.3], ["top_k", "top_p", "top_k"], [{"k": 7}, {"thres": 0.9}, None]
    one = [m.synthesis_sample_text2semantic(ids[j], temprature=temps[j], filter_logits_fn=fns[j], filter_fn_kwargs=kws[j], uniforms=us[j],
                                            return_logprobs=True) for j in range(3)]
    lst = m.synthesis_sample_text2semantic(ids, temprature=temps, filter_logits_fn=fns, filter_fn_kwargs=kws, uniforms=us, return_logprobs=True,
                                           slots=2)
    for j in range(3):
        assert _same(tuple(t.cpu() for t in lst[j]), tuple(t.cpu() for t in one[j])), (name, j)
    flat = m.synthesis_sample_text2semantic(ids, temprature=temps, filter_logits_fn=fns, filter_fn_kwargs=kws, uniforms=us)
    assert all(torch.equal(flat[j], one[j][0]) for j in range(3))
    # all-equal lists are the scalar call
    same = m.synthesis_sample_text2semantic(ids, temprature=[0.7] * 3, uniforms=us)
    scalar = m.synthesis_sample_text2semantic(ids, temprature=0.7, uniforms=us)
    assert all(torch.equal(a, b) for a, b in zip(same, scalar))
    # a prefix: the result starts with it and continues as the un-prefixed decode did
    pre = one[1][1][:, :5].cpu()
    cont = m.synthesis_sample_text2semantic(ids[1], temprature=temps[1], filter_logits_fn=fns[1], filter_fn_kwargs=kws[1], uniforms=us[1],
                                            return_logprobs=True, prefix=pre)
    if not bool((pre == V - 1).any()):
        assert _same(tuple(t.cpu() for t in cont), tuple(t.cpu() for t in one[1]))
    # best_of_temperatures: candidate c at temperature c, the candidate best_candidate picks among three decodes alone
    bt = (0.7, 1.0, 1.3)
    gen = torch.Generator().manual_seed(5)
    cu = [torch.rand(3, steps, S, V, generator=gen).clamp_(1e-6, 1 - 1e-6) for _ in range(2)]
    got = m.synthesis_sample_text2semantic(ids[:2], uniforms=cu, best_of_temperatures=bt, return_logprobs=True, slots=4)
    for j in range(2):
        cands = [m.synthesis_sample_text2semantic(ids[j], temprature=bt[k], uniforms=cu[j][k], return_logprobs=True) for k in range(3)]
        scores = [sequence_logprob(x[2], x[1], V - 1) for x in cands]
        assert len(set(scores)) == 3
        best = cands[best_candidate(scores)]
        assert _same(tuple(t.cpu() for t in got[j]), tuple(t.cpu() for t in best)), (name, j, scores)
    assert torch.equal(m.synthesis_sample_text2semantic(ids[0], uniforms=cu[0], best_of_temperatures=bt, best_of=3), got[0][0])
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], uniforms=cu[0], best_of_temperatures=bt, best_of=2)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids, temprature=[0.7, 1.0], uniforms=us)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic(ids[0], temprature=[0.7], uniforms=us[0])
    for bad in (dict(temprature=temps), dict(prefix=[None, pre, None]), dict(best_of_temperatures=bt)):
        with pytest.raises(ValueError):
            m.synthesis_sample_text2semantic(ids, beam_search_decode=True, beam_size=2, **bad)
    plain = CoVoMixModel(sd, hparams={"text2semantic": True}).eval().to(DEV)
    if S == 1:
        with pytest.raises(AssertionError):                 # the reference's assertion if ANY scale is > 1
            plain.synthesis_sample_text2semantic(ids, cond_scale=[1.0, 2.0, 1.0], uniforms=us)
        with pytest.raises(ValueError, match="two calls"):
            m.synthesis_sample_text2semantic(ids, cond_scale=[1.0, 2.0, 1.0], uniforms=us)


# ---------------------------------------------------------------- 9. CLI
def test_cli_side_files(tmp_path, monkeypatch):
    """three one-turn utterances; a.turn0.t2s.json (temperature, top_p) and b.turn0.prefix.semantic.npy: the decode stage hands the
    facade per-turn lists and the prefix, and every turn's tokens equal the run that gets the settings by flags / the facade call that
    gets the prefix; without the side files the facade is called exactly as it always was"""
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
    names = ["dlg_a", "dlg_b", "dlg_c"]
    for i, n in enumerate(names):
        for suf in ("_1", "_2"):
            np.save(os.path.join(pdir, f"{n}{suf}.hubert_code.npy"), rng.randint(0, 500, size=20))
            np.save(os.path.join(pdir, f"{n}{suf}.mel.npy"), (rng.randn(80, 20) * 2 - 6).astype(np.float32))
        np.save(os.path.join(tdir, f"{n}.turn0.text_ids.npy"), rng.randint(1, 199, size=(1, 7 + i)).astype(np.int64))
    real = generation.CoVoMixModel.synthesis_sample_text2semantic
    calls = []

    def spy(self, ids, **kw):
        res = real(self, ids, max_length=12, **kw)
        calls.append((self, [i.clone() for i in ids], kw, [r.cpu() for r in res]))
        return res
    monkeypatch.setattr(generation.CoVoMixModel, "synthesis_sample_text2semantic", spy)
    base = ["--t2s_ckpt", os.path.join(tmp, "t2s.ckpt"), "--acous_ckpt", os.path.join(tmp, "acous.ckpt"),
            "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"), "--text_dir", tdir, "--prompt_dir", pdir, "--mode", "covosingle"]
    flags = ["--t2s_temperature", "0.7", "--t2s_filter", "top_p", "--t2s_filter_thres", "0.8"]

    def run(out, extra=()):
        del calls[:]
        with pytest.warns(UserWarning, match="EMA"):
            assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, out)] + list(extra)) == 3
        assert len(calls) == 1
        return calls[0]

    _, ids0, kw0, plain = run("o0")                                        # no side files: the call of always
    assert set(kw0) == {"uniforms", "slots"}
    _, _, kwf, by_flags = run("o1", flags)                                 # the settings by flags, for all three
    assert kwf["temprature"] == 0.7 and kwf["filter_logits_fn"] == "top_p" and kwf["filter_fn_kwargs"] == {"thres": 0.8}
    assert not torch.equal(by_flags[0], plain[0]), "the flags changed nothing: the test cannot tell the settings apart"
    assert plain[1].numel() >= 6 and int(plain[1][:4].max()) < tsd["semantic_token_emb.weight"].shape[0] - 1
    with open(os.path.join(tdir, "dlg_a.turn0.t2s.json"), "w") as f:
        json.dump({"temperature": 0.7, "filter": "top_p", "filter_thres": 0.8}, f)
    np.save(os.path.join(tdir, "dlg_b.turn0.prefix.semantic.npy"), plain[1][:4].numpy())
    model, ids, kw, mixed = run("o2")
    assert kw["temprature"] == [0.7, 1.0, 1.0] and kw["filter_logits_fn"] == ["top_p", "top_k", "top_k"]
    assert kw["filter_fn_kwargs"] == [{"thres": 0.8}, None, None] and kw["cond_scale"] == [1.0] * 3
    assert [p is not None for p in kw["prefix"]] == [False, True, False]
    assert torch.equal(mixed[0], by_flags[0])                              # == the run that got them by flags
    assert torch.equal(mixed[2], plain[2]) and torch.equal(mixed[1], plain[1])      # (a prefix of its own tokens: the decode resumes)
    api = real(model, ids[1], uniforms=kw["uniforms"][1], max_length=12, prefix=torch.from_numpy(plain[1][:4].numpy()[None, :]))
    assert torch.equal(api.cpu(), mixed[1])
    other = torch.tensor([[3, 1, 4]])                                      # not its own tokens: the result starts with them
    np.save(os.path.join(tdir, "dlg_b.turn0.prefix.semantic.npy"), other[0].numpy())
    _, _, kw3, forced = run("o3")
    assert torch.equal(forced[1][:3], other[0]) and torch.equal(forced[0], by_flags[0])
    assert torch.equal(forced[1], real(model, ids[1], uniforms=kw3["uniforms"][1], max_length=12, prefix=other).cpu())
    # the flag: one temperature per candidate
    _, _, kwb, _ = run("o4", ["--t2s_best_of_temperatures", "0.7,1.0"])
    assert kwb["best_of_temperatures"] == (0.7, 1.0) and all(tuple(u.shape)[0] == 2 and u.ndim == 4 for u in kwb["uniforms"])
    os.remove(os.path.join(tdir, "dlg_a.turn0.t2s.json")); os.remove(os.path.join(tdir, "dlg_b.turn0.prefix.semantic.npy"))
    _, _, kw5, again = run("o5")                                           # the side files gone: today's files, byte for byte
    assert set(kw5) == {"uniforms", "slots"} and all(torch.equal(a, b) for a, b in zip(again, plain))
    files = [sorted(os.listdir(os.path.join(tmp, o))) for o in ("o0", "o2", "o5")]
    assert files[0] == files[1] == files[2] and "dlg_a.wav" in files[0]
    for f in files[0]:
        if f.endswith(".wav"):
            assert open(os.path.join(tmp, "o0", f), "rb").read() == open(os.path.join(tmp, "o5", f), "rb").read(), f
