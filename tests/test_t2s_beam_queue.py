"""CPU: beam search through continuously refilled slot groups (cvx_t2s_beam_queue_steps, TextToSemanticDecoder.generate_beam_many) - what can
be checked without a GPU: the argument checks that come before any device work, the ctypes struct against its field list, and the kernel
descriptors of the built library (the two new kernels keep everything in registers)."""
import ctypes as C

import pytest

from test_attention_form_d import _gfx950_kernel_descriptors


def _bare_decoder(max_length=40):
    """a decoder object without weights or device buffers: the argument checks must not get as far as needing them"""
    from covomix_amd.t2s import TextToSemanticDecoder
    model = object.__new__(TextToSemanticDecoder)
    model.max_length = max_length
    return model


def test_generate_beam_many_checks_its_arguments_before_any_device_work():
    import torch
    model = _bare_decoder()
    srcs = [torch.arange(1, 6)[None, :], torch.arange(1, 4)[None, :]]
    with pytest.raises(ValueError, match="limits"):
        model.generate_beam_many(srcs, beam_size=3, limits=[5])
    with pytest.raises(ValueError, match="limits"):
        model.generate_beam_many(srcs, beam_size=3, limits=[5, 6, 7])
    for bad in (0, -1, 17, 2.0, True):
        with pytest.raises(ValueError, match="beam_size"):
            model.generate_beam_many(srcs, beam_size=bad)
    with pytest.raises(ValueError, match="slots"):
        model.generate_beam_many(srcs, beam_size=10, slots=9)
    with pytest.raises(ValueError, match="slots"):
        model.generate_beam_many(srcs, beam_size=1, slots=0)
    with pytest.raises(ValueError, match="at least one step"):
        model.generate_beam_many(srcs, beam_size=3, max_length=-1)


def test_beam_queue_struct_matches_its_field_list():
    from covomix_amd import _lib
    pointers = ("queue", "utterances", "start", "parents", "hist_tokens", "hist_logprobs", "final_scores", "final_steps", "final_finished",
                "tokens", "logprobs")
    names = [f[0] for f in _lib.T2SBeamQueue._fields_]
    assert names == ["struct_size", "n_utterances"] + list(pointers)
    assert C.sizeof(_lib.T2SBeamQueue) == 4 + 4 + 8 * len(pointers) == 96
    assert _lib.T2SBeamQueue.struct_size.offset == 0 and _lib.T2SBeamQueue.queue.offset == 8
    ret, args = _lib.SIGNATURES["cvx_t2s_beam_queue_steps"]
    assert ret is C.c_int and args[:3] == [C.POINTER(_lib.T2SDecoder), C.POINTER(_lib.T2SBeam), C.POINTER(_lib.T2SBeamQueue)]
    assert _lib.ABI_VERSION == 113


def test_beam_queue_kernels_use_no_scratch():
    """read from the built library: the refilling merge kernel and the per-utterance back-track kernel have no private segment"""
    from covomix_amd import _lib
    kds = _gfx950_kernel_descriptors(_lib.LIB_PATH)
    merge = {k: v for k, v in kds.items() if "beam_merge_queue_kernel" in k}
    back = {k: v for k, v in kds.items() if "beam_backtrack_queue_kernel" in k}
    assert len(merge) == 1 and len(back) == 1, sorted(k for k in kds if "beam" in k)
    for name, (group, private, vgprs) in {**merge, **back}.items():
        print(f"FIGURE {name[:70]}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
        assert private == 0, (name, private)
