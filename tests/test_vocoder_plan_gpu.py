"""The HiFi-GAN host on the generator configurations that leave its stock route (tests/vocoder_plans.py: FALLBACK_CASES).

Every configuration the rest of the suite builds has upsample_initial_channel in {500, 64, 32} with the stock kernel and dilation lists: in
f16x3 all of them take the channels-last pipeline.  The four cases here reach, through Generator, the channel-major flow with split
ResBlocks between fp32 upsamplers, the polyphase upsampler's max|x| hand-over, ResBlocks pair by pair and convolution by convolution, a
stage whose ResBlocks stay on the fp32 kernels and an upsampler the split pipe refuses.  Frame counts 21 (3392 positions in the last
stage: several 256-position blocks and a ragged tail) and 3 (shorter than conv_pre's seven taps).  Bounds: those of
test_ragged_gpu.test_vocoder_ragged_batch_vs_b1_and_oracle (1e-6 from the item's own unbatched call, 1e-5 from the oracle - here the
oracle evaluated in fp64; the fp32 oracle itself sits 2.7e-7 to 1.2e-6 from it on these configurations)."""
import warnings

import pytest
import torch

from conftest import rel_l2
from vocoder_plans import COUNTED, FALLBACK_CASES, config, expected_calls

pytestmark = pytest.mark.gpu

FRAMES = [21, 3]


def _generator(h, **kw):
    import covomix_amd.synthetic as syn
    from covomix_amd.vocoder import AttrDict, Generator
    vsd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(syn.hifigan_param_shapes(h), seed=0).items()}
    gen = Generator(AttrDict(h), precision="f16x3", **kw).to("cuda:0")
    gen.load_state_dict(vsd); gen.eval(); gen.remove_weight_norm()
    return gen, vsd


def _mels(seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(80, t, generator=g) * 2 - 6).clamp(-11.52, 2.0) for t in FRAMES]


@pytest.mark.parametrize("case", list(FALLBACK_CASES))
def test_fallback_forms_ragged_vs_unbatched_and_fp64_oracle(case):
    import covomix_oracle as orc
    h = config(case)
    gen, vsd = _generator(h)
    folded = orc.fold_weight_norm(vsd)
    folded64 = {k: v.double() for k, v in folded.items()}
    mels = _mels(list(FALLBACK_CASES).index(case))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        wavs = [w.clone() for w in gen.ragged([m.cuda() for m in mels])]
        again = gen.ragged([m.cuda() for m in mels])
        singles = [gen(m.cuda()) for m in mels]
    for t, m, w, w2, single in zip(FRAMES, mels, wavs, again, singles):
        ref64 = orc.hifigan_forward(folded64, h, m[None].double())[0]
        ref32 = orc.hifigan_forward(folded, h, m[None])[0]
        e1, e2, e32 = rel_l2(w, single), rel_l2(w, ref64), rel_l2(ref32, ref64)
        print(f"FIGURE vocoder-plan {case} frames={t} ragged_vs_unbatched={e1:.3e} err_vs_fp64={e2:.3e} unbatched_vs_fp64={rel_l2(single, ref64):.3e} "
              f"fp32_oracle_vs_fp64={e32:.3e}")
        assert w.shape == single.shape == ref64.shape == (1, gen.output_length(t))
        assert e1 < 1e-6 and e2 < 1e-5, (case, t, e1, e2)
        assert torch.equal(w, w2)                                       # a second call: the same bits
    assert not any("saturat" in str(x.message) for x in rec)            # clamped log-mels never leave the window


@pytest.mark.parametrize("case,group", [(c, True) for c in FALLBACK_CASES] + [("stock", True), ("stock", False)])
def test_one_call_launches_what_the_plan_says(case, group, monkeypatch):
    """Recording pass-throughs around the ops front ends for ONE generator call: the counts must be those tests/vocoder_plans.py derives
    from the generator's plan (tests/test_vocoder_plan.py holds plan and table to literals)."""
    import covomix_amd.ops as ops_
    h = config(None if case == "stock" else case)
    gen, _ = _generator(h, group_stages=group)
    mel = torch.stack([m[:, :19] for m in (_mels(7)[0], _mels(8)[0])]).cuda()
    gen.pack()
    calls = dict.fromkeys(COUNTED, 0)

    def through(name):
        real = getattr(ops_, name)

        def fn(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        monkeypatch.setattr(ops_, name, fn)
    for name in COUNTED:
        through(name)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y = gen(mel, lengths=[19, 11])
    assert not any("saturat" in str(x.message) for x in rec)            # (a re-run on the fp32 twin would count twice)
    assert y.shape == (2, 1, gen.output_length(19)) and bool(torch.isfinite(y).all())
    want = dict(dict.fromkeys(COUNTED, 0), **expected_calls(gen.plan, h))
    assert calls == want, (gen.plan, {k: (calls[k], want[k]) for k in COUNTED if calls[k] != want[k]})
