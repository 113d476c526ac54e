"""CPU: the host side of the text2semantic prefill pass (t2s.prefill_rows, prefill_windows, the refusals, the ABI additions, the CLI
flag) and the fp32 restatement of its attention against the fp64 math of the oracle on the shapes of the GPU kernel test."""
import inspect
import os
import re

import pytest
import torch

import t2s_prefill_restated as rs
from conftest import ROOT


# ---------------------------------------------------------------- the attention definition
@pytest.mark.parametrize("heads", rs.HEADS)
@pytest.mark.parametrize("causal", [True, False])
def test_restated_attention_against_the_fp64_oracle(heads, causal):
    d = rs.description(heads)
    k, v, kbase = (d["k"], d["v"], d["cu"][:-1]) if causal else (d["kv"][:, :64 * heads], d["kv"][:, 64 * heads:], d["kbase_cross"])
    got = rs.restated(d["q"], k, v, d["cu"], kbase, d["nk"], heads, rs.SCALE, causal)
    ref = rs.oracle(d["q"], k, v, d["cu"], kbase, d["nk"], heads, causal)
    err = rs.rel_l2(got, ref, d["cu"], heads)
    print(f"heads {heads}, causal {causal}: largest rel-L2 per (sequence, head) {float(err.max()):.3e}")
    assert bool(torch.isfinite(got).all()) and float(err.max()) < rs.REL_L2
    # a row at position 0 of a causal sequence, and a sequence with one key, return that key's value
    if causal:
        assert torch.allclose(got[d["cu"][3]], v[d["cu"][3]], rtol=0, atol=1e-6)
    else:
        assert torch.allclose(got[d["cu"][0]], v[d["kbase_cross"][0]], rtol=0, atol=1e-6)


# ---------------------------------------------------------------- prefill_rows
def _seqs(S, V, lengths, records, ctxs, slots, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, V, (S, L), generator=g), r, c, s) for L, r, c, s in zip(lengths, records, ctxs, slots)]


def _hold(seqs, S, max_length, ctx_rows):
    from covomix_amd.t2s import prefill_rows
    t, ref = prefill_rows(seqs, S, max_length, ctx_rows), rs.rows_restated(seqs, S, max_length, ctx_rows)
    M = len(ref["rows"])
    assert t["rows"] == M and t["cu"].tolist() == ref["cu"] and t["cu"].dtype == torch.int32
    assert t["max_q"] == max(b - a for a, b in zip(ref["cu"], ref["cu"][1:]))
    assert t["positions"].tolist() == [r["pos"] for r in ref["rows"]] and t["positions"].dtype == torch.int64
    assert t["gather"].tolist() == [r["gather"] for r in ref["rows"]] and t["gather"].shape == (M, S)
    assert t["targets"].tolist() == [r["target"] for r in ref["rows"]]
    assert t["starts"].tolist() == [i for i, r in enumerate(ref["rows"]) if r["start"]] == ref["cu"][:-1]
    assert t["kbase"].tolist() == ref["kbase"] and t["nk"].tolist() == ref["nk"] and t["kbase"].dtype == t["nk"].dtype == torch.int32
    if ref["rows"][0]["cache"] is None:
        assert t["cache"] is None
    else:
        assert t["cache"].tolist() == [r["cache"] for r in ref["rows"]]
    return t


@pytest.mark.parametrize("S", [1, 2])
def test_prefill_rows_against_the_restatement(S):
    V, max_length, ctx_rows = 50, 24, 18
    lengths = [1, max_length, 7, 2]
    t = _hold(_seqs(S, V, lengths, [3, 0, 5, 1], [4, 18, 1, 9], [None] * 4), S, max_length, ctx_rows)
    assert t["cache"] is None
    # with slots: the cache rows of a sequence never leave its slot
    slots = [2, 0, 7, 5]
    t = _hold(_seqs(S, V, lengths, [2, 0, 7, 5], [4, 18, 1, 9], slots, seed=1), S, max_length, ctx_rows)
    cu = t["cu"].tolist()
    for i, s in enumerate(slots):
        rows = t["cache"][cu[i]:cu[i + 1]]
        assert int(rows.min()) == s * max_length and int(rows.max()) == s * max_length + lengths[i] - 1 < (s + 1) * max_length
    assert len(set(t["cache"].tolist())) == t["rows"]


def test_prefill_rows_guided_pairs():
    """a guided utterance is two sequences over the same tokens: its text half, and its null half with ctx = 1 in the record behind"""
    from covomix_amd.t2s import TextToSemanticDecoder
    tok = [torch.tensor([[5, 6, 7]]), torch.tensor([[1]]), torch.tensor([[2, 3]])]
    seqs, nulls = TextToSemanticDecoder._prefill_pairs(None, tok, [0, 2, 3], [9, 4, 6], [1.5, 1.0, 2.0], True)
    assert nulls == [3, -1, 4] and len(seqs) == 5
    assert [(s[1], s[2], s[3]) for s in seqs] == [(0, 9, 0), (2, 4, 2), (3, 6, 3), (1, 1, 1), (4, 1, 4)]
    assert torch.equal(seqs[3][0], tok[0]) and torch.equal(seqs[4][0], tok[2])
    t = _hold(seqs, 1, 8, 12)
    assert t["nk"].tolist() == [9, 4, 6, 1, 1] and t["kbase"].tolist() == [0, 24, 36, 12, 48]
    seqs, nulls = TextToSemanticDecoder._prefill_pairs(None, tok, [0, 1, 2], [9, 4, 6], [1.0, 1.0, 1.0], False)
    assert nulls == [-1, -1, -1] and all(s[3] is None for s in seqs)


def test_prefill_rows_refusals():
    from covomix_amd.t2s import prefill_rows
    ok = torch.zeros(1, 3, dtype=torch.int64)
    for seqs in ([], [(torch.zeros(1, 0, dtype=torch.int64), 0, 1, None)], [(torch.zeros(1, 9, dtype=torch.int64), 0, 1, None)],
                 [(torch.zeros(2, 3, dtype=torch.int64), 0, 1, None)], [(ok, 0, 0, None)], [(ok, 0, 13, None)], [(ok, -1, 1, None)],
                 [(ok, 0, 1, 0), (ok, 1, 1, None)], [(ok, 0, 1, -1)]):
        with pytest.raises(ValueError):
            prefill_rows(seqs, 1, 8, 12)


def test_prefill_windows_cut_on_utterance_boundaries_only():
    from covomix_amd.t2s import PREFILL_ROWS, prefill_windows
    assert PREFILL_ROWS == 32768
    assert prefill_windows([3, 3, 3, 9, 1], 6) == [(0, 2), (2, 3), (3, 4), (4, 5)]          # (9 > cap: a pass of its own, never cut)
    assert prefill_windows([600] * 64) == [(0, 54), (54, 64)]
    assert prefill_windows([2, 2, 2], 100, [2, 2, 2], 4) == [(0, 2), (2, 3)]                # the record window cuts as well
    assert prefill_windows([], 6) == []
    rows = [int(x) for x in torch.randint(1, 700, (300,), generator=torch.Generator().manual_seed(3))]
    wins = prefill_windows(rows, 4096)
    assert wins[0][0] == 0 and wins[-1][1] == 300 and all(a[1] == b[0] for a, b in zip(wins, wins[1:]))
    assert all(sum(rows[a:b]) <= 4096 for a, b in wins)
    assert all(sum(rows[a:b]) + rows[b] > 4096 for a, b in wins[:-1]), "a pass ends only where the next utterance would not fit"


# ---------------------------------------------------------------- refusals
def _bare(**d):
    from covomix_amd.t2s import TextToSemanticDecoder
    m = TextToSemanticDecoder.__new__(TextToSemanticDecoder)
    m.d = dict(streams=1, vocab=50, dim_target=64, dim_emb=64)
    m.d.update(d)
    m.max_length = 16
    return m


def test_refusals():
    from covomix_amd.t2s import check_prefixes
    m = _bare()
    with pytest.raises(ValueError, match="mixed_guidance"):
        m.generate_many([torch.ones(1, 3, dtype=torch.int64)], prefixes=[torch.zeros(1, 2, dtype=torch.int64)], mixed_guidance=True, prefill=True)
    with pytest.raises(ValueError, match="forced"):                          # a prefix for a forced utterance, as ever
        check_prefixes([torch.zeros(1, 2, dtype=torch.int64)], 1, 1, 50, [8], forced=[torch.zeros(1, 4, dtype=torch.int64)])
    m._prefill_check()
    for d in (dict(dim_target=66, dim_emb=66), dict(dim_target=132, dim_emb=66, streams=2)):
        with pytest.raises(ValueError, match="multiples of 4"):
            _bare(**d)._prefill_check()
        with pytest.raises(ValueError, match="multiples of 4"):              # ... before anything touches a device
            _bare(**d).score_many([torch.ones(1, 3, dtype=torch.int64)], [torch.zeros(d.get("streams", 1), 4, dtype=torch.int64)], prefill=True)


def test_the_switch_is_off_by_default_everywhere():
    from covomix_amd.conditional_model import CoVoMixModel
    from covomix_amd.t2s import TextToSemanticDecoder
    for fn in (TextToSemanticDecoder.score_many, TextToSemanticDecoder.generate_many, CoVoMixModel.score_text2semantic,
               CoVoMixModel.synthesis_sample_text2semantic):
        assert inspect.signature(fn).parameters["prefill"].default is False, fn


# ---------------------------------------------------------------- ABI and CLI
def test_header_binding_and_abi_version():
    import ctypes as C
    from covomix_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "covomix_hip.h")).read()
    assert re.search(r"int cvx_t2s_prefill_attention_f32\(const cvx_t2s_prefill_attention\* p, cvx_stream_t stream\);", hdr)
    assert re.search(r"int cvx_t2s_prefill_guidance_f32\(float\* logits, const int32_t\* null_row, const float\* scale, int64_t rows", hdr)
    assert re.search(r"#define CVX_ABI_VERSION 113\b", hdr) and _lib.ABI_VERSION == 113
    assert _lib.SIGNATURES["cvx_t2s_prefill_attention_f32"] == (C.c_int, [C.POINTER(_lib.T2SPrefillAttention), C.c_void_p])
    assert "cvx_t2s_prefill_guidance_f32" in _lib.SIGNATURES
    body = re.search(r"typedef struct cvx_t2s_prefill_attention \{(.*?)\} cvx_t2s_prefill_attention;", hdr, re.S).group(1)
    names = re.findall(r"[\s*,](\w+)(?=[,;])", body)
    assert names == [f[0] for f in _lib.T2SPrefillAttention._fields_], names
    assert C.sizeof(_lib.T2SPrefillAttention) == 104
    lib = _lib.load()
    assert hasattr(lib, "cvx_t2s_prefill_attention_f32") and lib.cvx_version() == 113


def test_prefill_kernels_use_no_scratch_and_have_names_of_their_own():
    from covomix_amd import _lib
    from test_attention_form_d import _gfx950_kernel_descriptors
    from test_t2s_code_objects import SYMBOL
    kds = {k: v for k, v in _gfx950_kernel_descriptors(_lib.LIB_PATH).items() if "t2s_prefill" in k}
    assert len(kds) == 2 and any("t2s_prefill_attention_kernel" in k for k in kds), sorted(kds)
    for name, (group, private, vgprs) in kds.items():
        print(f"FIGURE {name}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
        assert private == 0 and SYMBOL.fullmatch(name) is None, name


def test_cli_flag_parses_and_defaults_to_off():
    from covomix_amd import generation
    p = generation.build_parser()
    a = p.parse_args([])
    assert a.t2s_prefill is False and "prefill" not in generation.t2s_sampling_kwargs(a)
    a = p.parse_args(["--t2s_prefill"])
    assert a.t2s_prefill is True and generation.t2s_sampling_kwargs(a)["prefill"] is True
    with pytest.raises(ValueError):
        generation.t2s_sampling_kwargs(p.parse_args(["--t2s_prefill", "--t2s_mixed_guidance"]))
