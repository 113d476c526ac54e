"""GPU: guided and unguided utterances in one slot pool (cvx_t2s_decode_steps_mixed, generate_many(mixed_guidance=True), the facade and
the CLI flag).  Every comparison is EXACT: an utterance gets, bit for bit, the tokens and log-probs it gets alone with its settings,
whichever slots it ran in; and the slots it ran in are those the host replay of the scheduler (mixed_schedule) names."""
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
N, GOLD_G, GOLD_U = 20, 10, 13


def _guided(j):
    return j % 3 == 0 or j == GOLD_G


class Pool:
    """cosingle_small, 20 utterances - guided iff j % 3 == 0 or j == GOLD_G, the two golden ones among them - and every one's decode
    ALONE with its own scale, once"""

    def __init__(self):
        from covomix_amd.t2s import CHUNK, TextToSemanticDecoder
        self.g, sd = load_small("cosingle_small")
        self.model = TextToSemanticDecoder(sd, torch.device(DEV), max_length=256)
        self.V = self.g["uniforms"].shape[-1]
        self.gold = np.load(os.path.join(GOLDEN, "t2s_cosingle_small_cfg.npz"))
        self.cfg = float(self.gold["cond_scale"])
        assert self.cfg == 1.5
        self.srcs = _texts(self.g, N, seed=5)
        self.unis = [decode_uniforms(1, self.V, salt=100 + i) for i in range(N)]
        gen = torch.Generator().manual_seed(9)
        self.limits = [1, CHUNK, CHUNK + 1, CHUNK - 1, 2 * CHUNK, 2, 3 * CHUNK - 1] + \
            torch.randint(3, DECODE_STEPS + 1, (N - 7,), generator=gen).tolist()
        gu = torch.from_numpy(self.gold["uniforms"])[:, :, 0, :]
        self.srcs[GOLD_G], self.unis[GOLD_G], self.limits[GOLD_G] = torch.from_numpy(self.gold["source_ids"]), \
            torch.cat((gu, self.unis[GOLD_G][gu.shape[0]:])), gu.shape[0]
        uu = torch.from_numpy(self.g["uniforms"])[:, :, 0, :]
        self.srcs[GOLD_U], self.unis[GOLD_U], self.limits[GOLD_U] = torch.from_numpy(self.g["source_ids"]), \
            torch.cat((uu, self.unis[GOLD_U][uu.shape[0]:])), uu.shape[0]
        self.kinds = [_guided(j) for j in range(N)]
        assert self.kinds[GOLD_G] and not self.kinds[GOLD_U]
        self.scales = [self.cfg if k else 1.0 for k in self.kinds]
        self.sets = [{"cond_scale": s} for s in self.scales]
        self._alone = {}

    def alone(self, j, scale=None, **kw):
        """(flat, streams, logprobs) of utterance j alone, host tensors"""
        scale = self.scales[j] if scale is None else scale
        key = (j, scale, json.dumps(kw, sort_keys=True))
        if key not in self._alone:
            r = self.model.generate(self.srcs[j], uniforms=self.unis[j][:self.limits[j]], cond_scale=scale, return_logprobs=True, **kw)
            self._alone[key] = tuple(t.cpu() for t in r)
        return self._alone[key]


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    for scale in (1.0, p.cfg):                                   # (scale by scale: one captured graph at a time)
        for j in range(N):
            if p.scales[j] == scale:
                p.alone(j)
    return p


def _same(res, want):
    return len(res) == len(want) == 3 and all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(res, want))


def _idle(model, nb):
    st = model.buf["state"][:nb].cpu()
    return bool((st[:, 0] == model.max_length).all()) and bool((st[:, 7] == 0).all())


# ---------------------------------------------------------------- 1. the mixed pool == each alone
@pytest.mark.parametrize("slots", [2, 3, 8, 16])
def test_mixed_pool_equals_each_alone(pool, slots):
    from covomix_amd.t2s import mixed_schedule
    p, m = pool, pool.model
    done = []
    res = m.generate_many(p.srcs, p.unis, slots=slots, limits=p.limits, settings=p.sets, return_logprobs=True, mixed_guidance=True,
                          on_done=lambda j, r: done.append(j))
    rec = m.last_records
    assert sorted(done) == list(range(N)) and len(rec) == N
    for j in range(N):
        assert _same(res[j], p.alone(j)), (slots, j, rec[j])
        assert rec[j][4] == p.alone(j)[1].shape[1]
    assert torch.equal(res[GOLD_G][0], torch.from_numpy(p.gold["tokens"]))
    assert torch.equal(res[GOLD_U][0], torch.from_numpy(p.g["tokens"]))
    by_eos = sum(1 for r in rec if r[3] == 2)
    by_limit = sum(1 for r in rec if r[3] == 3)
    assert by_eos + by_limit == N and by_eos > 0 and by_limit > 0, (by_eos, by_limit)
    assert _idle(m, slots)
    sched = mixed_schedule(p.kinds, [r[4] for r in rec], slots)
    got = [(r[5], r[8]) for r in rec]
    print(f"{slots} slots: {by_eos} by eos, {by_limit} by limit; (slot, null slot, start): {sched}")
    assert got == [(s[0], s[1]) for s in sched]
    assert all((r[8] is None) == (not k) for r, k in zip(rec, p.kinds))
    if slots == 3:
        assert any(k and abs(r[5] - r[8]) > 1 for r, k in zip(rec, p.kinds)), got
    if slots >= 8:
        assert {s for g_ in got for s in g_ if s is not None} == set(range(slots))


# ---------------------------------------------------------------- 2. other behaviours
def test_scales_settings_and_prefixes(pool):
    """guided scales 1.5 / 2.0 / 3.0 beside unguided utterances with their own temperature and top-p, one prefixed utterance of each
    kind: each == alone"""
    p, m = pool, pool.model
    pick = list(range(10))
    scales = {0: 1.5, 3: 2.0, 6: 3.0, 9: 2.0}
    extra = {1: dict(temperature=0.7), 2: dict(filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.9}), 4: dict(temperature=1.3),
             3: dict(temperature=0.7, filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.8})}
    sets = [dict(cond_scale=scales.get(j, 1.0), **extra.get(j, {})) for j in pick]
    want = [p.alone(j, scales.get(j, 1.0), **extra.get(j, {})) for j in pick]
    # a prefix cut from the utterance's own result: the decode resumes and reproduces the rest
    pre = [None] * len(pick)
    for kind in (True, False):
        j = next(j for j in pick if (j in scales) == kind and want[j][1].shape[1] > 4 and not bool((want[j][1][:, :3] == p.V - 1).any()))
        pre[j] = want[j][1][:, :3]
    res = m.generate_many([p.srcs[j] for j in pick], [p.unis[j] for j in pick], slots=4, limits=[p.limits[j] for j in pick], settings=sets,
                          prefixes=pre, return_logprobs=True, mixed_guidance=True)
    for j in pick:
        assert _same(res[j], want[j]), (j, sets[j], pre[j] is not None, m.last_records[j])
    assert not torch.equal(want[3][1], p.alone(3)[1]) or not torch.equal(want[6][1], p.alone(6)[1]), "the scales did not arrive"
    # without scoring: the other instantiation of the sampling kernel
    res = m.generate_many([p.srcs[j] for j in pick], [p.unis[j] for j in pick], slots=5, limits=[p.limits[j] for j in pick], settings=sets,
                          prefixes=pre, mixed_guidance=True)
    for j in pick:
        assert len(res[j]) == 2 and torch.equal(res[j][0], want[j][0]) and torch.equal(res[j][1], want[j][1]), j
    with pytest.raises(ValueError, match="slots"):
        m.generate_many(p.srcs[:2], p.unis[:2], slots=1, settings=p.sets[:2], mixed_guidance=True)
    with pytest.raises(ValueError, match="cond_scale"):
        m.generate_many(p.srcs[:2], p.unis[:2], settings=[None, {"cond_scale": 0.5}], mixed_guidance=True)
    with pytest.raises(ValueError, match="two calls"):                    # the default path keeps its refusal
        m.generate_many(p.srcs[:2], p.unis[:2], settings=p.sets[:2])


def test_forced_logprobs_equal_sampled(pool):
    """one guided and one unguided FORCED utterance among sampled ones: their log-probs are those of the sampled decode of these tokens"""
    p, m = pool, pool.model
    pick = [4, 6, 7, 9]                                                   # 6, 9 guided
    forced = [None, p.alone(6)[1], p.alone(7)[1], None]
    res = m.generate_many([p.srcs[j] for j in pick], [p.unis[4], None, None, p.unis[9]], slots=3, limits=[p.limits[j] for j in pick],
                          settings=[p.sets[j] for j in pick], return_logprobs=True, forced=forced, mixed_guidance=True)
    for k, j in enumerate(pick):
        assert torch.equal(res[k][1], p.alone(j)[1]) and torch.equal(res[k][2], p.alone(j)[2]), j
    sc = m.score_many([p.srcs[6], p.srcs[7]], [p.alone(6)[1], p.alone(7)[1]], cond_scale=[p.cfg, 1.0], mixed_guidance=True)
    assert torch.equal(sc[0], p.alone(6)[2]) and torch.equal(sc[1], p.alone(7)[2])


def test_plain_launches_equal_graph_replay(pool, monkeypatch):
    p, m = pool, pool.model
    monkeypatch.setenv("CVX_GRAPH", "0")
    res = m.generate_many(p.srcs[:9], p.unis[:9], slots=4, limits=p.limits[:9], settings=p.sets[:9], return_logprobs=True, mixed_guidance=True)
    monkeypatch.setenv("CVX_GRAPH", "1")
    rep = m.generate_many(p.srcs[:9], p.unis[:9], slots=4, limits=p.limits[:9], settings=p.sets[:9], return_logprobs=True, mixed_guidance=True)
    for j in range(9):
        assert _same(res[j], p.alone(j)) and _same(rep[j], p.alone(j)), j
    assert sum(1 for k in m._graphs if k[0] == "mixed") >= 1


def test_all_of_one_kind_equals_todays_calls(pool):
    p, m = pool, pool.model
    n = 9
    for scale in (1.0, p.cfg):
        today = m.generate_many(p.srcs[:n], p.unis[:n], slots=4, limits=p.limits[:n], cond_scale=scale, return_logprobs=True)
        mixed = m.generate_many(p.srcs[:n], p.unis[:n], slots=4, limits=p.limits[:n], cond_scale=scale, return_logprobs=True, mixed_guidance=True)
        for j in range(n):
            assert _same(mixed[j], today[j]), (scale, j)
        assert all((r[8] is None) == (scale == 1.0) for r in m.last_records)


def test_two_output_model():
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_small("comix_small")
    m = TextToSemanticDecoder(sd, torch.device(DEV), max_length=256)
    S, V = g["uniforms"].shape[1], g["uniforms"].shape[-1]
    srcs = _texts(g, 5, seed=11)
    unis = [decode_uniforms(S, V, salt=300 + i)[:24] for i in range(5)]
    today = m.generate_many(srcs, unis, slots=2, return_logprobs=True)
    mixed = m.generate_many(srcs, unis, slots=2, return_logprobs=True, mixed_guidance=True, settings=[{"cond_scale": 1.0}] * 5)
    for j in range(5):
        assert _same(mixed[j], today[j]), j
    with pytest.raises(NotImplementedError):
        m.generate_many(srcs, unis, slots=2, mixed_guidance=True, settings=[None, None, {"cond_scale": 2.0}, None, None])
    with pytest.raises(NotImplementedError):
        m.generate_many(srcs, unis, slots=2, mixed_guidance=True, cond_scale=1.5)


# ---------------------------------------------------------------- 3. the C ABI directly
def _structs(m, n_guided=0, size=None):
    from covomix_amd import _lib
    per = _lib.T2SPerDialogue(C.sizeof(_lib.T2SPerDialogue), m.buf["per"].shape[0], m.buf["per"].data_ptr())
    mx = _lib.T2SMixed(C.sizeof(_lib.T2SMixed) if size is None else size, n_guided)
    return per, mx


def test_refusals_launch_nothing(pool):
    from covomix_amd import _lib, ops
    m, lib = pool.model, _lib.load()
    m._ensure(8, 8, 16, True)
    sentinel = torch.full_like(m.buf["state"], 5)          # position 5, role 5: a launch would advance it, write a token or re-arm it
    m.buf["state"].copy_(sentinel)
    m.buf["tokens"].fill_(3)
    m.buf["dialogues"].zero_()
    m.buf["queue"].copy_(torch.tensor([0, 8], dtype=torch.int32))
    queue0 = m.buf["queue"].clone()

    def call(n_guided=0, size=None, null_mixed=False, null_per=False, per_edit=None, scoring=None, steps=1, **edit):
        dec = m._descriptor(1.0, edit.pop("batch", 8), edit.pop("cfg_scale", 1.0), edit.pop("queue", True), None, edit.pop("nd", 8))
        for k, v in edit.items():
            setattr(dec, k, v)
        per, mx = _structs(m, n_guided, size)
        for k, v in (per_edit or {}).items():
            setattr(per, k, v)
        rc = lib.cvx_t2s_decode_steps_mixed(C.byref(dec), None if scoring is None else C.byref(scoring), None if null_per else C.byref(per),
                                            None if null_mixed else C.byref(mx), steps, ops._stream())
        torch.cuda.synchronize()
        return rc

    for steps in (0, 1):
        assert call(size=4, steps=steps) == EINVAL and call(size=16, steps=steps) == EINVAL and call(size=0, steps=steps) == EINVAL
        assert call(null_mixed=True, steps=steps) == EINVAL
        assert call(null_per=True, steps=steps) == EINVAL
        assert call(queue=False, nd=0, steps=steps) == EINVAL                         # dec->queue NULL
        assert call(cfg_scale=2.0, steps=steps) == EINVAL                             # the layout is per record here
        assert call(n_guided=-1, steps=steps) == EINVAL
        assert call(n_guided=5, steps=steps) == EINVAL                                # 2 * 5 > 8 records
        assert call(n_guided=1, batch=1, steps=steps) == EINVAL                       # a pair needs two slots
        assert call(n_guided=1, streams=2, steps=steps) == EINVAL                     # ... and a one-output model
        # what cvx_t2s_decode_steps_per_dialogue refuses
        assert call(per_edit=dict(struct_size=8), steps=steps) == EINVAL
        assert call(per_edit=dict(table=None), steps=steps) == EINVAL
        assert call(per_edit=dict(n_records=0), steps=steps) == EINVAL
        assert call(per_edit=dict(n_records=7), steps=steps) == EINVAL                # fewer rows than dialogue records
        assert call(scoring=_lib.T2SScoring(8, m.max_length, m.buf["logprobs"].data_ptr()), steps=steps) == EINVAL
        assert call(scoring=_lib.T2SScoring(16, m.max_length, None), steps=steps) == EINVAL
        assert call(scoring=_lib.T2SScoring(16, m.max_length - 1, m.buf["logprobs"].data_ptr()), steps=steps) == EINVAL
        assert call(batch=65, steps=steps) == EINVAL and call(state=None, steps=steps) == EINVAL
    assert call(steps=-1) == EINVAL
    assert torch.equal(m.buf["state"], sentinel) and bool((m.buf["tokens"] == 3).all())
    assert torch.equal(m.buf["queue"], queue0) and not bool(m.buf["dialogues"].any())
    # a valid call on idle slots with a drained queue launches and changes nothing
    m.buf["state"].copy_(m._slot_records([]))
    m.buf["queue"].copy_(torch.tensor([8, 8], dtype=torch.int32))
    assert call(n_guided=4, temperature=-1.0, filter_mode=5, top_k=0, top_p=2.0) == 0
    assert torch.equal(m.buf["state"].cpu(), m._slot_records([])) and bool((m.buf["tokens"] == 3).all())
    assert lib.cvx_version() == 113 == _lib.ABI_VERSION


@pytest.mark.parametrize("nb", [3, 8])
def test_zero_steps_arm_idle_slots(pool, nb):
    """n_steps == 0 on idle slots and queue = {0, n}: the scheduler alone.  Records G U G U U (7 records) - the slots, roles and records
    are those of mixed_schedule at start step 0, x holds the start token, the queue head stands behind the last record taken"""
    from covomix_amd import _lib, ops
    from covomix_amd.t2s import SR, mixed_records, mixed_schedule
    m, lib = pool.model, _lib.load()
    kinds = [True, False, True, False, False]
    first = mixed_records(kinds)
    nrec = first[-1]
    m._ensure(8, 8, 16)
    G = _lib.T2S_FLAG_GUIDED
    rec = torch.zeros(nrec, SR, dtype=torch.int32)
    for j, k in enumerate(kinds):
        rec[first[j]] = torch.tensor([5 + j, 9 + j, (G if k else 0) | (j & 1), 0, 0, 0, 0, 0], dtype=torch.int32)
        if k:
            rec[first[j] + 1] = torch.tensor([1, 9 + j, G | (j & 1), 0, 0, 0, 0, 0], dtype=torch.int32)
    m.buf["dialogues"].zero_()
    m.buf["dialogues"][:nrec].copy_(rec)
    m.buf["queue"].copy_(torch.tensor([0, nrec], dtype=torch.int32))
    idle = m._slot_records([])
    idle[2, 7], idle[7, 7] = 5, -1                                         # (a stale role on an idle slot of the batch is cleared or overwritten)
    m.buf["state"].copy_(idle)
    m.buf["x"].fill_(7.0)
    dec = m._descriptor(1.0, nb, 1.0, True, None, nrec)
    per, mx = _structs(m, sum(kinds))
    assert lib.cvx_t2s_decode_steps_mixed(C.byref(dec), None, C.byref(per), C.byref(mx), 0, ops._stream()) == 0
    torch.cuda.synchronize()
    sched = mixed_schedule(kinds, [1] * len(kinds), nb)
    taken = [j for j, s in enumerate(sched) if s is not None and s[2] == 0]
    assert taken == ([0, 1] if nb == 3 else [0, 1, 2, 3, 4])
    st, dl, x = m.buf["state"].cpu(), m.buf["dialogues"].cpu(), m.buf["x"].cpu()
    want = m._slot_records([])
    if nb == 3:
        want[7, 7] = -1                                                    # (outside the batch: not this call's slot)
    armed = set()
    for j in taken:
        s0, s1, _ = sched[j]
        r = first[j]
        want[s0] = torch.tensor([0, 0, 0, 5 + j, r, 9 + j, int(rec[r, 2]), 0 if s1 is None else s1 + 1], dtype=torch.int32)
        assert dl[r, 3] == 1 and dl[r, 5] == s0
        armed.add(s0)
        if s1 is not None:
            want[s1] = torch.tensor([0, 0, 0, 1, r + 1, 9 + j, int(rec[r, 2]), -(s0 + 1)], dtype=torch.int32)
            assert dl[r + 1, 3] == 1 and dl[r + 1, 5] == s1
            armed.add(s1)
    assert torch.equal(st, want), (st, want)
    head = first[taken[-1] + 1]
    assert m.buf["queue"].tolist() == [head, nrec]
    assert not bool(dl[head:nrec, 3].any())
    for s in range(8):
        assert torch.equal(x[s], m.start.cpu() if s in armed else torch.full_like(x[s], 7.0)), s


# ---------------------------------------------------------------- 4. facade and CLI
def test_facade_list_equals_one_by_one(pool):
    from covomix_amd.conditional_model import CoVoMixModel
    p = pool
    _, sd = load_small("cosingle_small")
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval().to(DEV)
    steps = 24
    ids, us = p.srcs[:5], [u[:steps] for u in p.unis[:5]]
    scales = [1.0, 2.0, 1.0, 1.5, 1.0]
    one = [m.synthesis_sample_text2semantic(ids[j], cond_scale=scales[j], uniforms=us[j], return_logprobs=True) for j in range(5)]
    lst = m.synthesis_sample_text2semantic(ids, cond_scale=scales, uniforms=us, return_logprobs=True, slots=3, mixed_guidance=True)
    for j in range(5):
        assert _same(tuple(t.cpu() for t in lst[j]), tuple(t.cpu() for t in one[j])), j
    flat = m.synthesis_sample_text2semantic(ids, cond_scale=scales, uniforms=us, slots=4, mixed_guidance=True)
    assert all(torch.equal(flat[j], one[j][0]) for j in range(5))
    sc = m.score_text2semantic(ids, [o[1] for o in one], cond_scale=scales, mixed_guidance=True)
    assert all(torch.equal(sc[j].cpu(), one[j][2].cpu()) for j in range(5))
    with pytest.raises(ValueError, match="two calls"):                    # the default stays
        m.synthesis_sample_text2semantic(ids, cond_scale=scales, uniforms=us)


def test_cli_flag_writes_the_same_files(tmp_path, monkeypatch):
    """three one-turn utterances whose side files make one of them guided: without the flag the decode stage makes two facade calls,
    with --t2s_mixed_guidance one - and the output directory holds the same files, byte for byte"""
    import covomix_amd.synthetic as syn
    from covomix_amd import generation
    from test_generation_gpu import _write_fixture
    tmp = str(tmp_path)
    _write_fixture(tmp, "vosingle")
    shapes = syn.t2s_param_shapes(two_output=False, dim=64, dim_target=64, source_depth=2, target_depth=2, heads=1, num_text=200)
    tsd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=0).items()}
    torch.save({"state_dict": {"cfm_wrapper.model." + k: v for k, v in tsd.items()},
                "hyper_parameters": {"text2semantic": True, "cond_drop_prob": 0.25}}, os.path.join(tmp, "t2s.ckpt"))
    tdir, pdir = os.path.join(tmp, "text"), os.path.join(tmp, "prompt")
    os.makedirs(tdir); os.makedirs(pdir)
    rng = np.random.RandomState(1)
    names = ["dlg_a", "dlg_b", "dlg_c"]
    for i, n in enumerate(names):
        for suf in ("_1", "_2"):
            np.save(os.path.join(pdir, f"{n}{suf}.hubert_code.npy"), rng.randint(0, 500, size=20))
            np.save(os.path.join(pdir, f"{n}{suf}.mel.npy"), (rng.randn(80, 20) * 2 - 6).astype(np.float32))
        np.save(os.path.join(tdir, f"{n}.turn0.text_ids.npy"), rng.randint(1, 199, size=(1, 7 + i)).astype(np.int64))
    with open(os.path.join(tdir, "dlg_b.turn0.t2s.json"), "w") as f:
        json.dump({"cond_scale": 2.0}, f)
    with open(os.path.join(tdir, "dlg_c.turn0.t2s.json"), "w") as f:
        json.dump({"temperature": 0.7}, f)
    real = generation.CoVoMixModel.synthesis_sample_text2semantic
    calls = []

    def spy(self, ids, **kw):
        res = real(self, ids, max_length=12, **kw)
        calls.append((kw, [r.cpu() for r in res]))
        return res
    monkeypatch.setattr(generation.CoVoMixModel, "synthesis_sample_text2semantic", spy)
    base = ["--t2s_ckpt", os.path.join(tmp, "t2s.ckpt"), "--acous_ckpt", os.path.join(tmp, "acous.ckpt"),
            "--hifigan_ckpt", os.path.join(tmp, "voc", "g_00000001"), "--text_dir", tdir, "--prompt_dir", pdir, "--mode", "covosingle"]

    def run(out, extra=()):
        del calls[:]
        with pytest.warns(UserWarning, match="EMA"):
            assert generation.run(True, base + ["--saved_dir", os.path.join(tmp, out)] + list(extra)) == 3
        return list(calls)

    two = run("two")
    assert len(two) == 2 and [kw["cond_scale"] for kw, _ in two] == [[1.0, 1.0], [2.0]]
    one = run("one", ["--t2s_mixed_guidance"])
    assert len(one) == 1 and one[0][0]["cond_scale"] == [1.0, 2.0, 1.0] and one[0][0]["mixed_guidance"] is True
    assert torch.equal(one[0][1][0], two[0][1][0]) and torch.equal(one[0][1][1], two[1][1][0]) and torch.equal(one[0][1][2], two[0][1][1])
    files = [sorted(os.listdir(os.path.join(tmp, o))) for o in ("two", "one")]
    assert files[0] == files[1] and "dlg_b.wav" in files[0]
    for f in files[0]:
        a, b = os.path.join(tmp, "two", f), os.path.join(tmp, "one", f)
        if os.path.isfile(a):
            assert open(a, "rb").read() == open(b, "rb").read(), f
