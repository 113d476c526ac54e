"""CPU: beam search under classifier-free guidance (cvx_t2s_beam_guided_steps, generate_beam(cond_scale=...)) - what needs no GPU.

  1. the guided oracle search (tests/t2s_beam_guided_restated.py) at scale 1 is the unguided one;
  2. the oracle alone meets the conditions the GPU cases rely on, asserted before any device is involved;
  3. the facade switch guided_beam and the CLI flag --t2s_beam_guided;
  4. the ABI: version 113, both prototypes in the header, both symbols exported and bound;
  5. the new kernels use no scratch (their LDS and VGPRs are printed)."""
import argparse
import os
import re

import pytest
import torch

import t2s_beam_guided_restated as bg
import t2s_beam_restated as br
from conftest import ROOT
from test_t2s_filters import load_small

ENTRIES = ("cvx_t2s_beam_guided_steps", "cvx_t2s_beam_guided_queue_steps")
NEW_KERNELS = ("beam_shortlist_guided_kernel", "beam_merge_guided_kernel", "beam_merge_guided_queue_kernel")


# ---------------------------------------------------------------- 1. scale 1 is the unguided oracle search
def test_guided_oracle_at_scale_one_is_the_unguided_oracle():
    g, sd = load_small("cosingle_small")
    src = torch.from_numpy(g["source_ids"])[:, :12]
    want = br.oracle_beam(sd, src, 3, bg.MAX_LEN)
    got = bg.oracle_beam_guided(sd, src, 3, bg.MAX_LEN, 1.0)
    assert len(got) == len(want)
    for t, (a, b) in enumerate(zip(got, want)):
        assert [(h[0], h[3], h[2]) for h in a["hyps"]] == [(h[0], h[3], h[2]) for h in b["hyps"]], t      # hypotheses and parents
        assert [h[1] for h in a["hyps"]] == [h[1] for h in b["hyps"]] and a["margin"] == b["margin"] and a["bound"] == b["bound"], t


# ---------------------------------------------------------------- 2. the oracle's side of the GPU cases
@pytest.mark.parametrize("ids,B,scale", bg.ORACLE_CASES)
def test_oracle_cases_are_decidable_and_re_parent(ids, B, scale):
    """measured: decidable prefixes of 14, 14 and 40 steps with 6, 8 and 33 re-parenting steps (12 ids, B = 3 at scale 3.0 reaches 4 steps
    only and is not used)"""
    g, sd = load_small("cosingle_small")
    steps, n, acc, moved = bg.oracle_case(sd, torch.from_numpy(g["source_ids"]), ids, B, scale)
    print(f"FIGURE {ids} ids, B = {B}, scale {scale}: decidable prefix {n} steps, {moved} of them re-parent, accumulated bound {acc[n - 1]:.3e}")
    assert n >= 12 and moved >= 4


@pytest.mark.parametrize("alpha,B,scale", bg.FINISHED_CASES)
def test_oracle_finished_cases(alpha, B, scale):
    """alpha 1.05: the search ends after 3 steps, hypotheses finishing at steps 0, 1, 2; alpha 0.95: three finish at 0, 1, 2 and are carried
    beside a live one to the step limit; every step decidable in both"""
    g, sd = load_small("cosingle_small")
    steps = bg.oracle_beam_guided(bg.with_eos_row(sd, alpha), torch.from_numpy(g["source_ids"]), B, bg.MAX_LEN, scale)
    n, _ = br.decidable_prefix(steps)
    fins = sorted(bg.first_finish(steps).values())
    print(f"FIGURE alpha {alpha}, B = {B}: {len(steps)} steps, ended {steps[-1]['ended']}, finishing at {fins}, decidable prefix {n}")
    assert n == len(steps) and fins[:3] == [0, 1, 2]
    if alpha > 1:
        assert steps[-1]["ended"] and len(steps) == 3
    else:
        assert not steps[-1]["ended"] and len(steps) == bg.MAX_LEN and len(fins) == 3


# ---------------------------------------------------------------- 3. facade and CLI
def test_facade_switch_without_a_gpu():
    from covomix_amd._lib import CovomixHipError
    from covomix_amd.conditional_model import CoVoMixModel
    g, sd = load_small("cosingle_small")
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval()
    ids = torch.from_numpy(g["source_ids"])
    kw = dict(beam_search_decode=True, max_length=8, cond_scale=1.5)
    with pytest.raises(NotImplementedError, match="guidance") as e:
        m.synthesis_sample_text2semantic(ids, **kw)                   # the default: refused as before
    assert "guided_beam" in str(e.value)
    with pytest.raises(NotImplementedError, match="guidance"):
        m.synthesis_sample_text2semantic(ids, guided_beam=False, **kw)
    with pytest.raises(CovomixHipError):                              # a valid call: there is no CPU path
        m.synthesis_sample_text2semantic(ids, guided_beam=True, **kw)
    with pytest.raises(CovomixHipError):                              # scale 1 with the switch: the plain beam call
        m.synthesis_sample_text2semantic(ids, guided_beam=True, beam_search_decode=True, max_length=8)
    for bad in (dict(best_of=2), dict(uniforms=torch.rand(8, 1, 502)), dict(prefix=torch.zeros(1, 2, dtype=torch.int64))):
        with pytest.raises(ValueError):                               # still no combination with beam search
            m.synthesis_sample_text2semantic(ids, guided_beam=True, **bad, **kw)
    with pytest.raises(ValueError):
        m.synthesis_sample_text2semantic([ids, ids], guided_beam=True, beam_search_decode=True, cond_scale=[1.5, 2.0], max_length=8)
    with pytest.raises(AssertionError, match="conditional drop"):     # the cond_drop_prob assertion applies unchanged
        CoVoMixModel(sd, hparams={"text2semantic": True}).eval().synthesis_sample_text2semantic(ids, guided_beam=True, **kw)
    g2, sd2 = load_small("comix_small")
    m2 = CoVoMixModel(sd2, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval()
    with pytest.raises(NotImplementedError, match="two-output"):
        m2.synthesis_sample_text2semantic(torch.from_numpy(g2["source_ids"]), guided_beam=True, **kw)


def test_beam_scale_check():
    from covomix_amd.t2s import check_beam_scale
    assert check_beam_scale(1) == 1.0 and check_beam_scale(2.5) == 2.5
    for bad in (0.5, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="cond_scale"):
            check_beam_scale(bad)


def test_cli_flag():
    from covomix_amd.generation import build_parser, t2s_sampling_kwargs
    base = dict(t2s_temperature=None, t2s_cond_scale=None, t2s_filter=None, t2s_filter_thres=None, t2s_top_k=None, t2s_best_of=1,
                t2s_beam_size=0)
    ns = lambda **kw: argparse.Namespace(**{**base, **kw})
    # a namespace without the attribute: the default
    assert t2s_sampling_kwargs(ns(t2s_beam_size=4)) == {"beam_search_decode": True, "beam_size": 4}
    with pytest.raises(ValueError, match="t2s_beam_size"):
        t2s_sampling_kwargs(ns(t2s_beam_size=4, t2s_cond_scale=1.5))
    with pytest.raises(ValueError, match="t2s_beam_size"):
        t2s_sampling_kwargs(ns(t2s_beam_size=4, t2s_cond_scale=1.5, t2s_beam_guided=False))
    assert t2s_sampling_kwargs(ns(t2s_beam_size=4, t2s_cond_scale=1.5, t2s_beam_guided=True)) == \
        {"cond_scale": 1.5, "beam_search_decode": True, "beam_size": 4, "guided_beam": True}
    assert t2s_sampling_kwargs(ns(t2s_beam_size=4, t2s_beam_guided=True)) == {"beam_search_decode": True, "beam_size": 4, "guided_beam": True}
    assert t2s_sampling_kwargs(ns(t2s_beam_guided=True)) == {}        # without beam search the flag adds nothing
    with pytest.raises(ValueError, match="t2s_beam_size"):
        t2s_sampling_kwargs(ns(t2s_beam_size=4, t2s_cond_scale=1.5, t2s_beam_guided=True, t2s_best_of=2))
    assert build_parser().parse_args(["--t2s_beam_guided"]).t2s_beam_guided is True and build_parser().parse_args([]).t2s_beam_guided is False


# ---------------------------------------------------------------- 4. the ABI
def test_abi_is_additive():
    from covomix_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "covomix_hip.h")).read()
    assert re.search(r"#define CVX_ABI_VERSION 113\b", hdr) and _lib.ABI_VERSION == 113
    lib = _lib.load()
    assert lib.cvx_version() == 113
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(const cvx_t2s_decoder\* dec, const cvx_t2s_beam\* beam, ", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES[ENTRIES[0]] == _lib.SIGNATURES["cvx_t2s_beam_steps"]
    assert _lib.SIGNATURES[ENTRIES[1]] == _lib.SIGNATURES["cvx_t2s_beam_queue_steps"]


# ---------------------------------------------------------------- 5. code objects
def test_new_kernels_use_no_scratch():
    from covomix_amd import _lib
    from test_attention_form_d import _gfx950_kernel_descriptors
    found = {}
    for name, (group, private, vgprs) in _gfx950_kernel_descriptors(_lib.LIB_PATH).items():
        m = re.fullmatch(r"_ZN12_GLOBAL__N_1\d+(" + "|".join(NEW_KERNELS) + r")E.*", name)
        if m:
            found[m.group(1)] = (group, private, vgprs)
    assert set(found) == set(NEW_KERNELS), sorted(set(NEW_KERNELS) - set(found))
    for name, (group, private, vgprs) in sorted(found.items()):
        print(f"FIGURE {name}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
        assert private == 0, (name, private)
