"""CPU: the beam search's selection step restated in fp64 and fp32 (tests/t2s_beam_restated.py) on crafted, decidable blocks; the
back-tracking of its records against a brute-force beam; the refusals of the facade and the CLI flags that need no GPU."""
import argparse
import math

import pytest
import torch

import t2s_beam_restated as br
import t2s_logprob_restated as rs
from test_t2s_filters import load_small


# ---------------------------------------------------------------- 1. the selection step, fp64 against fp32
@pytest.mark.parametrize("V", br.VOCABS)
def test_select_fp32_restatement_against_fp64(V):
    for B in br.BEAMS:
        for S in (1, 2):
            lg, sc, fin = br.block(B, S, V)
            assert br.decidable(lg, sc, fin, B), (B, S, V)            # before any fp32 result is looked at
            for G, rows in ((3, slice(0, 3 * B)), (1, slice(0, B)), (1, slice(B, 2 * B)), (1, slice(2 * B, 3 * B))):
                ref = br.select(lg[rows], sc[rows], fin[rows], B, torch.float64)
                got = br.select(lg[rows], sc[rows], fin[rows], B, torch.float32)
                what = (B, S, V, G, rows.start)
                assert torch.equal(got["parents"], ref["parents"]) and torch.equal(got["tokens"], ref["tokens"]), what
                assert torch.equal(got["finished"], ref["finished"]), what
                assert bool(((got["token_lp"].double() - ref["token_lp"]).abs() <= rs.bound(ref["token_lp"])).all()), what
                live = ref["scores"] > -math.inf
                assert torch.equal(got["scores"] > -math.inf, live), what
                assert bool(((got["scores"].double() - ref["scores"])[live].abs() <= 1e-4).all()), what
            ref = br.select(lg, sc, fin, B, torch.float64)
            K = min(B, V)
            # what the crafted groups are there for
            g0, g1, g2 = (slice(g * B, (g + 1) * B) for g in range(3))
            n0 = K ** S                                               # candidates of the one live hypothesis of the step-0 group
            assert int((ref["scores"][g1] > -math.inf).sum()) == min(B, n0) and bool((ref["parents"][g1][:min(B, n0)] == 0).all())
            assert bool((ref["tokens"][g1][min(B, n0):] == -1).all()) and bool((ref["finished"][g1][min(B, n0):] == 1).all())
            assert bool((ref["tokens"][g2] == -1).all()) and bool((ref["finished"][g2] == 1).all())
            assert sorted(ref["parents"][g2].tolist()) == list(range(B)), "all finished: every hypothesis carried once"
            if B >= 3:
                assert 2 in ref["parents"][g0].tolist(), "the finished hypothesis of the mixed group is kept"
            if B >= 2 and S == 1 and V >= B:
                p = ref["parents"][g0].tolist()
                if 0 in p and 1 in p:                                 # identical rows, equal scores: parent 0 first (the lower key)
                    assert p.index(0) < p.index(1)


def test_select_orders_ties_by_the_candidate_key():
    """equal logits inside a row: the shortlist takes the lowest indices; equal candidates: the lowest q"""
    B, V = 3, 5
    lg = torch.zeros(B, 1, V)
    sc = torch.tensor([0.0, 0.0, -1.0])
    r = br.select(lg, sc, torch.zeros(B, dtype=torch.uint8), B)
    assert r["parents"].tolist() == [0, 0, 0] and r["tokens"][:, 0].tolist() == [0, 1, 2]
    lg2 = torch.zeros(B, 2, V)
    r = br.select(lg2, sc, torch.zeros(B, dtype=torch.uint8), B)
    assert r["parents"].tolist() == [0, 0, 0] and r["tokens"].tolist() == [[0, 0], [0, 1], [0, 2]]
    lg[:, :, V - 1] = 10.0                                            # the eos on top: two finish, then hypothesis 0 with the next entry
    r = br.select(lg, torch.tensor([0.0, 0.0, -20.0]), torch.zeros(B, dtype=torch.uint8), B)
    assert r["tokens"][:, 0].tolist() == [V - 1, V - 1, 0] and r["parents"].tolist() == [0, 1, 0] and r["finished"].tolist() == [1, 1, 0]


# ---------------------------------------------------------------- 2. back-tracking
@pytest.mark.parametrize("T,B,S", [(1, 1, 1), (7, 3, 1), (40, 10, 2), (33, 16, 2)])
def test_backtrack_against_a_brute_force_beam(T, B, S):
    from covomix_amd.t2s import beam_backtrack
    gen = torch.Generator().manual_seed(T * 100 + B)
    parents = torch.randint(0, B, (T, B), generator=gen, dtype=torch.int32)
    tokens = torch.randint(0, 502, (T, B, S), generator=gen, dtype=torch.int32)
    lps = -torch.rand(T, B, S, generator=gen)
    want = br.brute_force_sequences(parents, tokens, lps)
    for i in range(B):
        tk, lp, path = beam_backtrack(parents, tokens, lps, i, T)
        assert tk.T.tolist() == want[i][0] and torch.equal(lp.T, torch.tensor(want[i][1])), (T, B, S, i)
        assert path[-1] == i and all(path[t] == int(parents[t + 1, path[t + 1]]) for t in range(T - 1))
    steps = br.replay(parents, tokens, lps)
    assert [list(map(list, steps[-1][i][0])) for i in range(B)] == [w[0] for w in want]


def test_beam_rank():
    from covomix_amd.t2s import beam_rank
    sc, ln = [-6.0, -2.0, -math.inf, -3.0], [6, 1, 0, 3]
    assert beam_rank(sc, ln, 1, 0.0) == [1, 3, 0, 2]                 # the raw score
    assert beam_rank(sc, ln, 1, 1.0) == [0, 3, 1, 2]                 # per token: -1, -1 (tie: the lower slot), -2
    assert beam_rank(sc, ln, 2, 1.0) == [0, 3, 1, 2]


# ---------------------------------------------------------------- 3. refusals that need no GPU
def test_facade_refusals_without_a_gpu():
    from covomix_amd._lib import CovomixHipError
    from covomix_amd.conditional_model import CoVoMixModel
    from covomix_amd.t2s import check_beam_size
    g, sd = load_small("cosingle_small")
    m = CoVoMixModel(sd, hparams={"cond_drop_prob": 0.25, "text2semantic": True}).eval()
    ids = torch.from_numpy(g["source_ids"])
    kw = dict(beam_search_decode=True, max_length=8)
    with pytest.raises(ValueError, match="uniforms"):
        m.synthesis_sample_text2semantic(ids, uniforms=torch.rand(8, 1, 502), **kw)
    with pytest.raises(ValueError, match="generator"):
        m.synthesis_sample_text2semantic(ids, generator=torch.Generator(), **kw)
    with pytest.raises(ValueError, match="best_of"):
        m.synthesis_sample_text2semantic(ids, best_of=2, **kw)
    for bad in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="beam_size"):
            m.synthesis_sample_text2semantic(ids, beam_size=bad, **kw)
        with pytest.raises(ValueError):
            check_beam_size(bad)
    with pytest.raises(NotImplementedError, match="guidance"):
        m.synthesis_sample_text2semantic(ids, cond_scale=1.5, **kw)
    with pytest.raises(CovomixHipError):                              # a valid call: there is no CPU path
        m.synthesis_sample_text2semantic(ids, **kw)
    assert check_beam_size(1) == 1 and check_beam_size(16) == 16


def test_cli_flag_refusals():
    from covomix_amd.generation import t2s_sampling_kwargs
    base = dict(t2s_temperature=None, t2s_cond_scale=None, t2s_filter=None, t2s_filter_thres=None, t2s_top_k=None, t2s_best_of=1,
                t2s_beam_size=0)
    ns = lambda **kw: argparse.Namespace(**{**base, **kw})
    assert t2s_sampling_kwargs(ns()) == {}                            # 0: sampling, nothing added
    assert t2s_sampling_kwargs(ns(t2s_beam_size=4)) == {"beam_search_decode": True, "beam_size": 4}
    for bad in (dict(t2s_beam_size=4, t2s_best_of=2), dict(t2s_beam_size=4, t2s_cond_scale=1.5), dict(t2s_beam_size=17),
                dict(t2s_beam_size=-1)):
        with pytest.raises(ValueError, match="t2s_beam_size"):
            t2s_sampling_kwargs(ns(**bad))
