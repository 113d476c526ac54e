"""CPU: the text2semantic logit filters (top-k with any k, top-p; reference text2semantic.py:118-132).
  * tests/t2s_filter_restated.py reproduces the masks the REFERENCE's own `top_k` / `top_p` gave the rows of
    tests/golden/t2s_filters.npz (tests/golden/make_golden_t2s_filters.py) exactly, for every row and setting;
  * host-side validation of the settings (t2s.filter_setting) and the --t2s_* command-line flags;
  * the caps the GPU tests of tests/test_t2s_filters_gpu.py rely on hold in fp64 alone: the share of fixture rows whose top-2 score
    margin is inside DELTA, and the share of undecidable steps of a filtered decode (on the CPU oracle's logits, with the oracle
    module's `top_k_filter` substituted)."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import t2s_filter_restated as rs

BLOCKS = (503, 1024)
TEMPS = (1.0, 0.7)
UNIFORM_SEED = 20240            # draws of the stand-alone sampling test (CPU check below: <= 2 % of the rows inside the margin)
DECODE_SEED = 77                # draws of the filtered decodes
DECODE_STEPS = 64
DECODE_FILTERS = {"top_p0.9": ("top_p", {"thres": 0.9}), "top_k7": ("top_k", {"k": 7})}


def fixture_block(V):
    g = np.load(os.path.join(GOLDEN, "t2s_filters.npz"))
    sets = [(str(n), int(m), int(k), float(t)) for n, m, k, t in zip(g[f"names_{V}"], g[f"mode_{V}"], g[f"k_{V}"], g[f"thres_{V}"])]
    return torch.from_numpy(g[f"logits_{V}"]), torch.from_numpy(g[f"kept_{V}"]), sets


def fixture_uniforms(V, rows):
    gen = torch.Generator().manual_seed(UNIFORM_SEED + V)
    return torch.rand(rows, V, generator=gen).clamp_(1e-6, 1 - 1e-6)


def decode_uniforms(S, V, salt=0):
    gen = torch.Generator().manual_seed(DECODE_SEED + salt)
    return torch.rand(DECODE_STEPS, S, V, generator=gen).clamp_(1e-6, 1 - 1e-6)


def load_small(name):
    g = np.load(os.path.join(GOLDEN, f"t2s_{name}.npz"))
    return g, {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w::")}


@pytest.mark.parametrize("V", BLOCKS)
def test_restatement_reproduces_the_reference_masks(V):
    logits, kept, sets = fixture_block(V)
    assert logits.shape[1] == V and kept.shape == (len(sets), logits.shape[0], V)
    names = [s[0] for s in sets]
    assert names == ["top_k k=1", "top_k k=51", f"top_k k={V}", "top_k thres=0.25", "top_p thres=0.5", "top_p thres=0.9", "top_p thres=0.99"]
    for i, (name, mode, k, thres) in enumerate(sets):
        got = rs.kept_mask(logits, mode, k, thres)
        assert torch.equal(got, kept[i]), (V, name, int((got != kept[i]).sum()))
        f = rs.filtered(logits, mode, k, thres)
        assert torch.equal(f > float("-inf"), kept[i]) and torch.equal(f[kept[i]], logits[kept[i]])


def test_ties():
    """what torch.topk / torch.sort leave open: top-k keeps every entry that equals the k-th largest (rank counting, as the decode
    always has); top-p counts equal logits as sorted by ascending index"""
    l = torch.tensor([[0.0, 2.0, 2.0, 2.0, -1.0]])
    assert rs.kept_mask(l, rs.TOP_K, 2).tolist() == [[False, True, True, True, False]]
    assert rs.kept_mask(l, rs.TOP_K, 4).tolist() == [[True, True, True, True, False]]
    p = torch.softmax(l.double(), -1)[0]
    assert rs.kept_mask(l, rs.TOP_P, 0, float(p[1]) + 1e-9).tolist() == [[False, True, True, False, False]]
    assert rs.kept_mask(l, rs.TOP_P, 0, float(p[1]) - 1e-9).tolist() == [[False, True, False, False, False]]


@pytest.mark.parametrize("V", BLOCKS)
def test_fixture_rows_inside_the_margin_are_rare(V):
    """what the GPU test may leave unchecked: rows whose top-2 score margin is inside DELTA - at most 2 % over all settings and
    temperatures, from fp64 alone"""
    logits, kept, sets = fixture_block(V)
    u = fixture_uniforms(V, logits.shape[0])
    n = bad = 0
    for i in range(len(sets)):
        for T in TEMPS:
            ok = rs.margin_ok(rs.score_of(logits, u, kept[i], T))
            n += ok.numel()
            bad += int((~ok).sum())
    print(V, "rows inside the margin:", bad, "of", n)
    assert bad <= 0.02 * n


def test_filter_setting_validation():
    from covomix_amd.t2s import filter_setting
    V = 502
    assert filter_setting(vocab=V) == (0, 51, 0.0)
    assert filter_setting("top_k", {"thres": 0.25}, V) == (0, 126, 0.0)
    assert filter_setting("top_k", {"k": 7, "thres": 0.5}, V) == (0, 7, 0.0)
    assert filter_setting("top_k", {"k": V}, V) == (0, V, 0.0)
    assert filter_setting("top_p", None, V) == (1, 0, 0.9)
    assert filter_setting("top_p", {"thres": 0.5}, V) == (1, 0, 0.5)
    for fn, kw in (("top_k", {"k": 0}), ("top_k", {"k": V + 1}), ("top_k", {"thres": 0.0}), ("top_p", {"thres": 0.0}),
                   ("top_p", {"thres": 1.0}), ("top_p", {"thres": 1.5}), ("top_p", {"k": 3}), ("top_a", None), ("top_k", {"p": 1})):
        with pytest.raises(ValueError):
            filter_setting(fn, kw, V)


def test_cli_flags_become_keywords():
    from covomix_amd import generation
    p = generation.build_parser()
    assert generation.t2s_sampling_kwargs(p.parse_args([])) == {}
    a = p.parse_args(["--t2s_temperature", "0.7", "--t2s_cond_scale", "1.5", "--t2s_filter", "top_p", "--t2s_filter_thres", "0.8"])
    assert generation.t2s_sampling_kwargs(a) == dict(temprature=0.7, cond_scale=1.5, filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.8})
    a = p.parse_args(["--t2s_top_k", "7"])
    assert generation.t2s_sampling_kwargs(a) == dict(filter_fn_kwargs={"k": 7})
    with pytest.raises(ValueError):
        generation.t2s_sampling_kwargs(p.parse_args(["--t2s_filter", "top_p", "--t2s_top_k", "7"]))
    with pytest.raises(SystemExit):
        p.parse_args(["--t2s_filter", "top_a"])


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
@pytest.mark.parametrize("filt", list(DECODE_FILTERS))
def test_filtered_decode_is_mostly_decidable_on_the_oracle(name, filt):
    """The CPU oracle's decode with its `top_k_filter` replaced by the restated filter: at most 5 % of its steps are undecidable
    for restated_choice (the cap the GPU test of the same decode uses), and at the decidable ones the oracle took that token."""
    import t2s_oracle as orc
    g, sd = load_small(name)
    fn, kw = DECODE_FILTERS[filt]
    S, V = g["uniforms"].shape[1], g["uniforms"].shape[-1]
    mode, k, thres = rs.setting(fn, V, **kw)
    uni = decode_uniforms(S, V)
    with mock.patch.object(orc, "top_k_filter", lambda logits, thres_=None: rs.filtered(logits, mode, k, thres)):
        o = orc.generate(sd, torch.from_numpy(g["source_ids"]), uni[:, :, None, :], max_length=DECODE_STEPS)
    logits = o["logits"][:, :, 0, :]                                   # [L, S, V]
    L = logits.shape[0]
    tokens, decidable = rs.restated_choice(logits, uni[:L], 1.0, mode, k, thres)
    streams = o["streams"][0].T                                        # [L, S]
    print(name, filt, "steps", L, "undecidable", int((~decidable).sum()))
    assert torch.equal(tokens[decidable], streams[decidable])
    assert int((~decidable).sum()) <= 0.05 * decidable.numel()
