"""vocoder.plan on the CPU: the plan of every generator configuration the suite builds, field for field against literals, and the call
table of tests/vocoder_plans.py on those plans (tests/test_vocoder_plan_gpu.py holds the table to what a generator call launches)."""
import pytest

from vocoder_plans import FALLBACK_CASES, config, expected_calls

STOCK_LENGTHS = [(5, 1), (20, 4), (80, 16), (160, 32)]          # rates 5 4 4 2, kernels 8 8 4 4: 160 T + 32 samples
RATE10_LENGTHS = [(10, 0), (40, 0), (80, 0), (160, 0)]          # rates 10 4 2 2, kernels 20 8 4 4
STOCK_UPS, RATE10_UPS = [(5, 8), (4, 8), (4, 4), (2, 4)], [(10, 20), (4, 8), (2, 4), (2, 4)]
CALLS3 = ("call", "call", "call")


def _stages(channels, ups, lengths, upsampler, forms):
    """forms: per stage (resblocks, blocks, np, wide)"""
    from covomix_amd.vocoder import Stage
    return tuple(Stage(c, u, k, upsampler, rb, blocks, np_, wide, mul, add)
                 for c, (u, k), (mul, add), (rb, blocks, np_, wide) in zip(channels, ups, lengths, forms))


def _fp32(channels, ups=STOCK_UPS, lengths=STOCK_LENGTHS):
    return _stages(channels, ups, lengths, "polyphase", [("fp32", (), None, False)] * 4)


def _narrow(blocks, np_=32):
    return ("blocks", blocks, np_, False)


MIXED = ("pairs", "call", "call")
EXPECTED = {
    # (configuration, precision, group_stages) -> (pipeline, cp_in, stages)
    ("stock500", "f16x3", True): ("channels_last", 512, lambda: _stages(
        [250, 125, 62, 31], STOCK_UPS, STOCK_LENGTHS, "split",
        [("grouped", CALLS3, 256, True), ("grouped", CALLS3, 128, True), _narrow(CALLS3, 64), _narrow(CALLS3)])),
    ("stock500", "f16x3", False): ("channels_last", 512, lambda: _stages(
        [250, 125, 62, 31], STOCK_UPS, STOCK_LENGTHS, "split",
        [("blocks", CALLS3, 256, True), ("blocks", CALLS3, 128, True), _narrow(CALLS3, 64), _narrow(CALLS3)])),
    ("stock64", "f16x3", True): ("channels_last", 64, lambda: _stages([32, 16, 8, 4], STOCK_UPS, STOCK_LENGTHS, "split", [_narrow(CALLS3)] * 4)),
    ("stock32", "f16x3", True): ("channels_last", 32, lambda: _stages([16, 8, 4, 2], STOCK_UPS, STOCK_LENGTHS, "split", [_narrow(CALLS3)] * 4)),
    ("stock500", "fp32", True): ("channel_major", None, lambda: _fp32([250, 125, 62, 31])),
    ("stock64", "fp32", True): ("channel_major", None, lambda: _fp32([32, 16, 8, 4])),
    ("stock32", "fp32", True): ("channel_major", None, lambda: _fp32([16, 8, 4, 2])),
    ("narrow_pairs", "f16x3", True): ("channel_major", None, lambda: _stages(
        [16, 8, 4, 2], STOCK_UPS, STOCK_LENGTHS, "polyphase", [_narrow(MIXED)] * 4)),
    ("wide_convs", "f16x3", True): ("channel_major", None, lambda: _stages(
        [128, 64, 32, 16], STOCK_UPS, STOCK_LENGTHS, "polyphase",
        [("blocks", ("convs", "call", "call"), 128, True), _narrow(MIXED, 64), _narrow(MIXED), _narrow(MIXED)])),
    ("fp32_blocks", "f16x3", True): ("channel_major", None, lambda: _fp32([16, 8, 4, 2])),
    ("rate10", "f16x3", True): ("channel_major", None, lambda: _stages(
        [16, 8, 4, 2], RATE10_UPS, RATE10_LENGTHS, "polyphase", [_narrow(CALLS3)] * 4)),
    ("rate10", "fp32", True): ("channel_major", None, lambda: _fp32([16, 8, 4, 2], RATE10_UPS, RATE10_LENGTHS)),
}

# one generator call on that plan: ops front end -> calls (the other counted front ends: none)
EXPECTED_CALLS = {
    ("stock500", "f16x3", True): dict(hifigan_conv1d=1, amax_pow2_scale=4, hifigan_to_channels_last=1, hifigan_conv_transpose1d_f16x3=4,
                                      pow2_scale_from_amax=4, hifigan_split_channels_last=5, hifigan_resblock_stage_f16x3=2,
                                      hifigan_resblock_f16x3=6, hifigan_post_channels_last=1),
    ("stock500", "f16x3", False): dict(hifigan_conv1d=1, amax_pow2_scale=4, hifigan_to_channels_last=1, hifigan_conv_transpose1d_f16x3=4,
                                       pow2_scale_from_amax=4, hifigan_split_channels_last=5, hifigan_resblock_f16x3=12,
                                       hifigan_post_channels_last=1),
    ("stock64", "f16x3", True): dict(hifigan_conv1d=1, amax_pow2_scale=4, hifigan_to_channels_last=1, hifigan_conv_transpose1d_f16x3=4,
                                     pow2_scale_from_amax=4, hifigan_split_channels_last=3, hifigan_resblock_f16x3=12, hifigan_post_channels_last=1),
    ("stock500", "fp32", True): dict(hifigan_conv1d=1 + 4 * 18, hifigan_conv_transpose1d=4, hifigan_post=1),
    ("narrow_pairs", "f16x3", True): dict(hifigan_conv1d=1, hifigan_conv_transpose1d=4, pow2_scale_from_amax=4, hifigan_to_channels_last=4,
                                          hifigan_from_channels_last=4, hifigan_resblock_pair_f16x3=8, hifigan_resblock_f16x3=8, hifigan_post=1),
    ("wide_convs", "f16x3", True): dict(hifigan_conv1d=1, hifigan_conv_transpose1d=4, pow2_scale_from_amax=4, hifigan_to_channels_last=4,
                                        hifigan_from_channels_last=4, hifigan_conv1d_f16x3=4, hifigan_resblock_pair_f16x3=6,
                                        hifigan_resblock_f16x3=8, hifigan_post=1),
    ("fp32_blocks", "f16x3", True): dict(hifigan_conv1d=1 + 4 * 18, hifigan_conv_transpose1d=4, hifigan_post=1),
    ("rate10", "f16x3", True): dict(hifigan_conv1d=1, hifigan_conv_transpose1d=4, pow2_scale_from_amax=4, hifigan_to_channels_last=4,
                                    hifigan_from_channels_last=4, hifigan_resblock_f16x3=12, hifigan_post=1),
}


def _config(name):
    return config(name) if name in FALLBACK_CASES else config(upsample_initial_channel=int(name[len("stock"):]))


@pytest.mark.parametrize("name,precision,group", list(EXPECTED), ids=[f"{n}-{p}-{'grouped' if g else 'plain'}" for n, p, g in EXPECTED])
def test_plan_field_for_field(name, precision, group):
    from covomix_amd import vocoder
    pipeline, cp_in, stages = EXPECTED[(name, precision, group)]
    p = vocoder.plan(_config(name), precision, group_stages=group)
    assert p == vocoder.Plan(pipeline, stages(), cp_in)
    if group:
        assert p == vocoder.plan(_config(name), precision)               # grouping is the default


@pytest.mark.parametrize("name,precision,group", list(EXPECTED_CALLS), ids=[f"{n}-{p}-{'grouped' if g else 'plain'}" for n, p, g in EXPECTED_CALLS])
def test_call_table_on_the_plans(name, precision, group):
    from covomix_amd import vocoder
    h = _config(name)
    assert expected_calls(vocoder.plan(h, precision, group_stages=group), h) == EXPECTED_CALLS[(name, precision, group)]


def test_one_width_rule_and_one_narrow_limit():
    """ops.hifigan_tile is the kernels' tile rule (32 / 64 / 128 / 256 columns), ops.HIFI_NARROW_NP the widest fused-pair stage"""
    from covomix_amd import ops
    assert [ops.hifigan_tile(c) for c in (1, 32, 33, 64, 65, 128, 129, 250, 256)] == [32, 32, 64, 64, 128, 128, 256, 256, 256]
    assert ops.HIFI_NARROW_NP == 64
    with pytest.raises(AssertionError):
        ops.hifigan_tile(257)


def test_a_rate_one_upsampler_is_zero_stuffed_and_its_split_stage_measures_its_own_maximum():
    from covomix_amd import vocoder
    h = config(upsample_initial_channel=32, upsample_rates=[1, 4], upsample_kernel_sizes=[3, 8], resblock_dilation_sizes=[[1, 3], [1, 3, 5], [1]])
    p = vocoder.plan(h, "f16x3")
    assert p.pipeline == "channel_major" and [st.upsampler for st in p.stages] == ["stuffed", "polyphase"]
    assert [(st.mul, st.add) for st in p.stages] == [(1, 0), (4, 0)] and all(st.blocks == ("pairs", "call", "pairs") for st in p.stages)
    calls = expected_calls(p, h)
    assert calls["hifigan_conv1d"] == 2 and calls["amax_pow2_scale"] == 1 and calls["pow2_scale_from_amax"] == 1
    assert calls["hifigan_resblock_pair_f16x3"] == 2 * 3 and calls["hifigan_resblock_f16x3"] == 2
