"""Shared by tests/test_vocoder_plan.py (CPU) and tests/test_vocoder_plan_gpu.py: the generator configurations that leave the stock
route of the HiFi-GAN host, and how many calls of each ops front end ONE generator call makes on a given vocoder.Plan.  Restated from
the forward code of covomix_amd.vocoder with no import of its logic: expected_calls reads nothing but the fields of the plan and the
dilation lists of the configuration.

  channels-last pipeline   conv_pre, max|x| and one converter into the first upsampler's input pair; per stage the split-pipe upsampler
                           (leaves max|x0|), its pre-scale, on a wide stage the split of x0, the ResBlocks, and - but for the last stage -
                           max|xs| and the split of xs into the next upsampler's input pair; conv_post reads the last xs channels-last
  channel-major flow       conv_pre; per stage the polyphase upsampler (its own front end) or the zero-stuffed one (the fp32
                           convolution); a split stage then takes its pre-scale from the maximum the polyphase upsampler left, or measures
                           it, and sits between the two layout converters; an fp32 stage is two fp32 convolutions per dilation; conv_post
  ResBlocks of a stage     'grouped': one call for the stage; otherwise per block 'call' (one C call), 'pairs' (one fused kernel per
                           dilation) or 'convs' (two split-pipe convolutions per dilation)"""
import collections

FALLBACK_CASES = {
    "narrow_pairs": dict(upsample_initial_channel=32, resblock_dilation_sizes=[[1, 3], [1, 3, 5], [1, 3, 5]]),
    "wide_convs": dict(upsample_initial_channel=256, resblock_dilation_sizes=[[1, 3], [1, 3, 5], [1, 3, 5]]),
    "fp32_blocks": dict(upsample_initial_channel=32, resblock_kernel_sizes=[3, 7, 13]),
    "rate10": dict(upsample_initial_channel=32, upsample_rates=[10, 4, 2, 2], upsample_kernel_sizes=[20, 8, 4, 4]),
}


def config(name=None, **overrides):
    """synthetic.HIFIGAN_COVOMIX_CONFIG with the overrides of the named fallback case (and / or the given ones)"""
    import covomix_amd.synthetic as syn
    h = dict(syn.HIFIGAN_COVOMIX_CONFIG)
    h.update(FALLBACK_CASES[name] if name else {})
    h.update(overrides)
    return h


def expected_calls(plan, h):
    """front end name -> calls during one Generator call that does not saturate"""
    n = collections.Counter()
    dils = [len(d) for d in h["resblock_dilation_sizes"]]
    cl = plan.pipeline == "channels_last"
    n["hifigan_conv1d"] += 1                                          # conv_pre
    if cl:
        n["amax_pow2_scale"] += 1
        n["hifigan_to_channels_last"] += 1
    for i, st in enumerate(plan.stages):
        assert (st.upsampler == "split") == cl
        n[{"split": "hifigan_conv_transpose1d_f16x3", "polyphase": "hifigan_conv_transpose1d", "stuffed": "hifigan_conv1d"}[st.upsampler]] += 1
        if st.resblocks == "fp32":
            n["hifigan_conv1d"] += 2 * sum(dils)
            continue
        n["amax_pow2_scale" if st.upsampler == "stuffed" else "pow2_scale_from_amax"] += 1
        if cl:
            n["hifigan_split_channels_last"] += int(st.wide) + int(i + 1 < len(plan.stages))
            n["amax_pow2_scale"] += int(i + 1 < len(plan.stages))
        else:
            n["hifigan_to_channels_last"] += 1
            n["hifigan_from_channels_last"] += 1
        if st.resblocks == "grouped":
            n["hifigan_resblock_stage_f16x3"] += 1
            continue
        assert st.resblocks == "blocks" and len(st.blocks) == len(dils)
        for form, d in zip(st.blocks, dils):
            name, calls = {"call": ("hifigan_resblock_f16x3", 1), "pairs": ("hifigan_resblock_pair_f16x3", d),
                           "convs": ("hifigan_conv1d_f16x3", 2 * d)}[form]
            n[name] += calls
    n["hifigan_post_channels_last" if cl else "hifigan_post"] += 1
    return dict(n)


COUNTED = ("hifigan_conv1d", "hifigan_conv_transpose1d", "hifigan_conv_transpose1d_f16x3", "hifigan_conv1d_f16x3", "hifigan_conv1d_group_f16x3",
           "hifigan_resblock_f16x3", "hifigan_resblock_stage_f16x3", "hifigan_resblock_pair_f16x3", "hifigan_split_channels_last",
           "hifigan_to_channels_last", "hifigan_from_channels_last", "hifigan_post", "hifigan_post_channels_last", "amax_pow2_scale",
           "pow2_scale_from_amax")
