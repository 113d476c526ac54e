"""CPU: the text2semantic oracle (oracle/t2s_oracle.py) against the golden vectors the REFERENCE TextToSemantic produced
in the build container (tests/golden/make_golden_t2s.py): sampled tokens from the recorded uniform draws (bit-exact),
teacher-forced logits and encoder output (<= 1e-5 rel-L2).  SURVEY.md section 8f row N1."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2

import t2s_oracle as orc
import covomix_amd.synthetic as syn

KW = {
    "cosingle": dict(two_output=False, dim=512, dim_target=512),
    "comix": dict(two_output=True, dim=512, dim_target=1024),
}


def load_case(name):
    g = np.load(os.path.join(GOLDEN, f"t2s_{name}.npz"))
    if name.endswith("_small"):
        sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w::")}
    else:
        sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(**KW[name]), seed=0).items()}
    return g, sd


def test_t2s_param_counts_match_reference_probe():
    n = lambda s: sum(int(np.prod(v)) for v in s.values())
    assert n(syn.t2s_param_shapes(**KW["cosingle"])) == 45_287_312          # SURVEY section 8c probe
    assert n(syn.t2s_param_shapes(**KW["comix"])) == 76_758_584


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small", "cosingle", "comix"])
def test_t2s_oracle_vs_reference_golden(name):
    g, sd = load_case(name)
    src = torch.from_numpy(g["source_ids"])
    uni = torch.from_numpy(g["uniforms"])
    torch.set_num_threads(8)
    o = orc.generate(sd, src, uni, max_length=uni.shape[0])
    assert torch.equal(o["tokens"], torch.from_numpy(g["tokens"]))
    assert torch.equal(o["streams"], torch.from_numpy(g["streams"]))
    assert int(o["streams"][0, :, -1].max()) == 501                  # every fixture ends with a sampled eos
    of = orc.generate(sd, src, uni, forced=torch.from_numpy(g["streams"]))
    assert rel_l2(of["logits"], torch.from_numpy(g["logits"])) < 1e-5
    assert rel_l2(orc.encode(sd, src)[0], torch.from_numpy(g["encoder"])) < 1e-5


@pytest.mark.parametrize("name", ["cosingle_small", "cosingle"])
def test_t2s_oracle_guidance_vs_reference_golden(name):
    """Classifier-free guidance (text2semantic.py:780-792): the tokens the REFERENCE (built with cond_drop_prob > 0) sampled at
    cond_scale = 1.5 from the recorded draws, reproduced bit-exactly; they differ from the unguided run's."""
    _, sd = load_case(name)
    g = np.load(os.path.join(GOLDEN, f"t2s_{name}_cfg.npz"))
    src, uni = torch.from_numpy(g["source_ids"]), torch.from_numpy(g["uniforms"])
    torch.set_num_threads(8)
    o = orc.generate(sd, src, uni, max_length=uni.shape[0], cond_scale=float(g["cond_scale"]))
    assert torch.equal(o["tokens"], torch.from_numpy(g["tokens"])) and int(o["streams"][0, 0, -1]) == 501
    assert not torch.equal(orc.generate(sd, src, uni, max_length=uni.shape[0])["tokens"], o["tokens"])


def test_t2s_helpers():
    t = torch.tensor([[5, 7, 0, 0], [3, 4, 6, 9]])
    out = orc.set_eos_id(t.clone(), 99, 0)
    assert out.tolist() == [[5, 7, 99, 0, 0], [3, 4, 6, 9, 99]]
    m = orc.mask_after_eos(torch.tensor([[1, 501, 7, 8], [2, 3, 4, 501]]), 501, -1)
    assert m.tolist() == [[1, 501, -1, -1], [2, 3, 4, 501]]
    f = orc.top_k_filter(torch.arange(502, dtype=torch.float32)[None])
    assert int(torch.isfinite(f).sum()) == 51 and bool(torch.isfinite(f[0, -51:]).all())


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small", "cosingle", "comix"])
def test_teacher_forced_pass_vs_reference_golden_and_stepwise(name):
    """teacher_forced_logits (one causal full-sequence pass, fp64 after the fp32 rotary angle) against the reference's teacher-forced
    logits and against the step-by-step `generate(forced=...)` run in fp64; reference_choice picks the reference's tokens."""
    g, sd = load_case(name)
    src, streams = torch.from_numpy(g["source_ids"]), torch.from_numpy(g["streams"])
    torch.set_num_threads(8)
    tf = orc.teacher_forced_logits(sd, src, streams[0])
    ref = torch.from_numpy(g["logits"])[:, :, 0]
    assert tf.dtype == torch.float64 and tf.shape == ref.shape
    assert rel_l2(tf, ref) < 1e-5
    stepwise = orc.generate({k: v.double() for k, v in sd.items()}, src, None, forced=streams)["logits"][:, :, 0]
    assert rel_l2(tf, stepwise) < 1e-9
    assert float(orc.per_position_rel_l2(tf, stepwise).max()) < 1e-9
    tokens, decidable = orc.reference_choice(tf, torch.from_numpy(g["uniforms"])[:, :, 0])
    assert torch.equal(tokens.T, streams[0]) and float(decidable.float().mean()) > 0.95


@pytest.mark.parametrize("name", ["cosingle_small", "cosingle"])
def test_teacher_forced_guidance_vs_reference_golden(name):
    """cond_scale > 1: the combined logits of the fp64 pass against the step-by-step oracle (pinned to the reference's guided
    tokens), and the reference's guided tokens from reference_choice."""
    _, sd = load_case(name)
    g = np.load(os.path.join(GOLDEN, f"t2s_{name}_cfg.npz"))
    src, uni, scale = torch.from_numpy(g["source_ids"]), torch.from_numpy(g["uniforms"]), float(g["cond_scale"])
    torch.set_num_threads(8)
    o = orc.generate({k: v.double() for k, v in sd.items()}, src, uni.double(), max_length=uni.shape[0], cond_scale=scale)
    tf = orc.teacher_forced_logits(sd, src, o["streams"][0], cond_scale=scale)
    assert rel_l2(tf, o["logits"][:, :, 0]) < 1e-9
    tokens, decidable = orc.reference_choice(tf, uni[:, :, 0])
    assert torch.equal(tokens[:, 0], torch.from_numpy(g["tokens"])) and bool(decidable.all())


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_long_tolerance_sees_one_lost_key_and_the_last_context_row(name):
    """The per-position tolerance of tests/test_t2s_long_gpu.py (LONG_LOGIT_TOL) flags, at EVERY later position, a decode that lost
    one self-attention key (position 1000 of 1100: one lost 64-key block loses more) or the last context row (the text eos: an
    off-by-one in the key count) - the long GPU checks can see either."""
    _, sd = load_case(name)
    g = np.load(os.path.join(GOLDEN, f"t2s_{name}.npz"))
    src = torch.from_numpy(g["source_ids"])
    S, L = g["streams"].shape[1], 1100
    streams = torch.randint(0, 501, (S, L), generator=torch.Generator().manual_seed(0))
    torch.set_num_threads(8)
    base = orc.teacher_forced_logits(sd, src, streams)
    keep = torch.ones(L, dtype=torch.bool)
    keep[1000] = False
    e = orc.per_position_rel_l2(orc.teacher_forced_logits(sd, src, streams, self_mask=keep), base)
    print(name, "key 1000 lost: min rel-L2 after it", float(e[1001:].min()))
    assert float(e[:1000].max()) == 0.0 and float(e[1000:].min()) > 3 * orc.LONG_LOGIT_TOL
    ctx = torch.ones(src.shape[-1] + 1, dtype=torch.bool)
    ctx[-1] = False
    e = orc.per_position_rel_l2(orc.teacher_forced_logits(sd, src, streams, context_mask=ctx), base)
    print(name, "last context row lost: min rel-L2", float(e.min()))
    assert float(e.min()) > 3 * orc.LONG_LOGIT_TOL
    e32 = orc.per_position_rel_l2(orc.teacher_forced_logits(sd, src, streams, dtype=torch.float32), base)
    assert float(e32.max()) < orc.LONG_LOGIT_TOL / 3           # while fp32 arithmetic alone stays well inside it


def test_reference_choice_decidability():
    """reference_choice: the top-k + Gumbel argmax in fp64, and the steps it refuses to call (a runner-up within delta, or an entry
    within delta of the top-k boundary that could win if it crossed it)."""
    V, k = 20, 2                                        # ceil(0.1 * 20) = 2
    lg = torch.zeros(4, 1, V, dtype=torch.float64)
    u = torch.full((4, 1, V), math.exp(-1.0), dtype=torch.float64)           # gumbel_from_uniform = 0 everywhere
    lg[0, 0, 3], lg[0, 0, 7] = 5.0, 4.0                                        # clear winner 3
    lg[1, 0, 3], lg[1, 0, 7] = 5.0, 5.0 - 1e-4                                 # runner-up too close
    lg[2, 0, 3], lg[2, 0, 7], lg[2, 0, 9] = 5.0, 1.0, 1.0 - 1e-4               # boundary tie between 7 and 9, neither can win
    lg[3, 0, 3], lg[3, 0, 7], lg[3, 0, 9] = 5.0, 1.0, 1.0 - 1e-4
    u[3, 0, 9] = 1.0 - 1e-12                                                   # ... but 9 would win if it were in the set
    tokens, dec = orc.reference_choice(lg, u)
    assert tokens[:, 0].tolist() == [3, 3, 3, 3]
    assert dec[:, 0].tolist() == [True, False, True, False]
    ref = orc.top_k_filter(lg[:, 0]) + orc.gumbel_from_uniform(u[:, 0])
    assert torch.equal(tokens[:, 0], ref.argmax(dim=-1))
    hot, _ = orc.reference_choice(lg, u, temperature=1e-3)                    # temperature divides the filtered logits only
    assert hot[:, 0].tolist() == [3, 3, 3, 3]
