"""CPU: the host side of the text2semantic log-probabilities - sequence_logprob, the best-of-N selection and its tie rule, the
arguments score_many and best_of refuse, the --t2s_best_of flag and its seeds, and the fp32 restatement of the log-prob epilogue
against fp64 on the rows the GPU test uses (tests/t2s_logprob_restated.py)."""
import math

import pytest
import torch

import t2s_logprob_restated as rs

EOS = 9


def test_sequence_logprob_hand_made():
    from covomix_amd.t2s import sequence_logprob
    # no eos: every position counts
    assert sequence_logprob(torch.tensor([[-1.0, -2.0, -3.0]]), torch.tensor([[1, 2, 3]]), EOS) == pytest.approx(-2.0)
    # an eos at position 0: that position alone (what follows is padding)
    assert sequence_logprob(torch.tensor([[-0.5, -7.0, -9.0]]), torch.tensor([[EOS, 1, EOS]]), EOS) == pytest.approx(-0.5)
    # two streams that end at different steps: 2 + 4 positions
    lp = torch.tensor([[-1.0, -2.0, -100.0, -100.0], [-1.0, -1.0, -1.0, -3.0]])
    st = torch.tensor([[4, EOS, 5, 6], [1, 2, 3, EOS]])
    assert sequence_logprob(lp, st, EOS) == pytest.approx((-3.0 - 6.0) / 6)
    # an eos in one stream only: 1 + 3 positions
    lp = torch.tensor([[-4.0, -50.0, -50.0], [-1.0, -2.0, -3.0]])
    st = torch.tensor([[EOS, 0, 0], [1, 2, 3]])
    assert sequence_logprob(lp, st, EOS) == pytest.approx((-4.0 - 6.0) / 4)
    # fp32 log-probs are summed in fp64; a [L] pair is one stream
    assert sequence_logprob(torch.tensor([-1.0, -2.0]), torch.tensor([1, EOS]), EOS) == pytest.approx(-1.5)
    with pytest.raises(ValueError):
        sequence_logprob(torch.zeros(1, 3), torch.zeros(1, 4, dtype=torch.int64), EOS)
    with pytest.raises(ValueError):
        sequence_logprob(torch.zeros(1, 0), torch.zeros(1, 0, dtype=torch.int64), EOS)


def test_best_of_selection_and_ties():
    from covomix_amd.t2s import best_candidate, sequence_logprob
    assert best_candidate([-3.0, -1.0, -2.0]) == 1
    assert best_candidate([-1.0, -1.0, -2.0]) == 0            # the lowest index wins ties
    assert best_candidate([-2.0, -1.0, -1.0]) == 1
    assert best_candidate([-5.0]) == 0
    assert best_candidate([float("nan"), -9.0, -9.0]) == 1    # a NaN never beats a number
    with pytest.raises(ValueError):
        best_candidate([])
    # on made-up log-prob tensors: candidate 2 is the most likely per token although candidate 0 has the largest SUM
    lps = [torch.tensor([[-1.0, -1.0]]), torch.tensor([[-0.9, -0.9, -0.9, -3.0]]), torch.tensor([[-0.5, -0.6, -0.7, -0.8]])]
    sts = [torch.tensor([[1, EOS]]), torch.tensor([[1, 2, 3, EOS]]), torch.tensor([[1, 2, 3, 4]])]
    scores = [sequence_logprob(l, s, EOS) for l, s in zip(lps, sts)]
    assert best_candidate(scores) == 2
    assert best_candidate([scores[0], scores[0], scores[1]]) == 0


def test_best_of_arguments():
    from covomix_amd.t2s import check_best_of
    assert check_best_of(1) == 1 and check_best_of(4) == 4
    for bad in (0, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            check_best_of(bad)
    u = torch.rand(3, 8, 1, 16)
    assert check_best_of(3, None, u) == 3 and check_best_of(3, 2, [u, u]) == 3
    assert check_best_of(1, None, torch.rand(8, 1, 16)) == 1           # best_of = 1: today's [steps, S, V]
    with pytest.raises(ValueError):
        check_best_of(2, None, u)                                       # [3, ...] draws for 2 candidates
    with pytest.raises(ValueError):
        check_best_of(3, None, torch.rand(8, 1, 16))                    # no candidate dimension
    with pytest.raises(ValueError):
        check_best_of(3, 2, [u])                                        # one tensor for two utterances


def test_score_many_refuses_bad_targets():
    from covomix_amd.t2s import check_targets
    S, V, M = 2, 502, 40
    ok = check_targets([torch.zeros(2, 1, dtype=torch.int64), torch.full((2, 40), V - 1)], S, V, M)
    assert [tuple(t.shape) for t in ok] == [(2, 1), (2, 40)] and all(t.dtype == torch.int64 for t in ok)
    assert tuple(check_targets([torch.arange(5)], 1, V, M)[0].shape) == (1, 5)          # [L] is one stream
    for bad in (torch.zeros(2, 0, dtype=torch.int64),                  # L < 1
                torch.zeros(2, 41, dtype=torch.int64),                 # L > max_length
                torch.full((2, 3), V),                                 # a token == vocab
                torch.tensor([[0, -1, 3], [0, 1, 2]]),                 # the pad id
                torch.zeros(1, 3, dtype=torch.int64),                  # one stream for a two-output model
                torch.zeros(2, 3, 1, dtype=torch.int64),
                torch.zeros(2, 3)):                                    # floats
        with pytest.raises(ValueError):
            check_targets([ok[0], bad], S, V, M)


def test_cli_best_of_flag_and_seeds():
    from covomix_amd import generation
    p = generation.build_parser()
    assert p.parse_args([]).t2s_best_of == 1
    assert generation.t2s_sampling_kwargs(p.parse_args([])) == {}
    assert generation.t2s_sampling_kwargs(p.parse_args(["--t2s_best_of", "1"])) == {}             # 1 = off: today's call
    assert generation.t2s_sampling_kwargs(p.parse_args(["--t2s_best_of", "4"])) == {"best_of": 4}
    a = p.parse_args(["--t2s_best_of", "2", "--t2s_filter", "top_p"])
    assert generation.t2s_sampling_kwargs(a) == {"best_of": 2, "filter_logits_fn": "top_p"}
    with pytest.raises(ValueError):
        generation.t2s_sampling_kwargs(p.parse_args(["--t2s_best_of", "0"]))
    # candidate 0 keeps the seed the single decode has always had; the others depend on c only and collide with nothing in use
    assert generation._candidate_salt(0) == 1
    assert generation._stable_seed(30, "dlg_a", 3, generation._candidate_salt(0)) == generation._stable_seed(30, "dlg_a", 3, 1)
    salts = [generation._candidate_salt(c) for c in range(8)]
    assert len(set(salts)) == 8 and 2 not in salts                      # (2: the acoustic noise)
    assert len({generation._stable_seed(30, "dlg_a", 3, s_) for s_ in salts}) == 8


@pytest.mark.parametrize("V", rs.VOCABS)
def test_fp32_restatement_meets_the_bound(V):
    """the inputs of the GPU test are decidable: fp32 arithmetic in three summation orders stays within a TENTH of the bound"""
    lg, tk = rs.rows_for(V)
    ref = rs.reference(lg, tk)
    assert lg.shape == (tk.shape[0], V) and bool(torch.isfinite(ref).all())
    for order in rs.SUMS:
        u = rs.ulps(rs.restated(lg, tk, order), ref)
        print(V, order, f"{float(u.max()):.2f} units of 2^-24 (1 + |lp|)")
        assert float(u.max()) <= rs.LOGP_TOL_ULPS / 10, (V, order)
    assert math.isclose(float(rs.bound(torch.tensor(0.0, dtype=torch.float64))), 256 * 2.0 ** -24)
