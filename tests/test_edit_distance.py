"""CPU: the host side of the edit-distance call (ops.edit_distance over cvx_edit_distance_i64) and what is built on it -
  1. the restatement (edit_distance_restated.py) against the textbook matrix, and the metric properties;
  2. the table builder against the package's, and every refusal of the host layer and of the entry point's host checks;
  3. counted_tokens against sequence_logprob's counting;
  4. consensus_candidate and token_error_rate on hand-made cases;
  5. the CLI flag, the facade's ValueErrors, the header and the binding (ABI version still 113)."""
import ctypes as C
import inspect
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import edit_distance_restated as rs

EINVAL = -22


# ---------------------------------------------------------------- 1. the restatement
def test_restatement_against_the_textbook_matrix():
    """exhaustive over a 3-symbol alphabet up to length 5 against length <= 5 (364 x 364 pairs would be slow: every a against a sample of
    b), then 3000 random pairs of lengths 0..12"""
    words = [w for n in range(6) for w in itertools.product(range(3), repeat=n)]
    rng = np.random.RandomState(0)
    for a in words:
        for k in rng.randint(0, len(words), size=12):
            assert rs.distance(a, words[k]) == rs.naive(a, words[k]), (a, words[k])
    for _ in range(3000):
        a, b = (rng.randint(0, 3, size=rng.randint(0, 13)) for _ in range(2))
        assert rs.distance(a, b) == rs.naive(a, b), (a, b)


def test_restatement_is_a_metric():
    rng = np.random.RandomState(1)
    for _ in range(300):
        al = int(rng.choice([2, 3, 501]))
        a, b, c = (rng.randint(0, al, size=rng.randint(0, 40)) for _ in range(3))
        ab, ba, bc, ac = rs.distance(a, b), rs.distance(b, a), rs.distance(b, c), rs.distance(a, c)
        assert ab == ba and ac <= ab + bc and rs.distance(a, a) == 0
        assert abs(len(a) - len(b)) <= ab <= max(len(a), len(b))
    assert rs.distance([], []) == 0 and rs.distance([], [5, 5]) == 2 and rs.distance([1, 2, 3], []) == 3
    assert rs.distance([1, 2, 3, 4], [4, 3, 2, 1]) == 4 and rs.distance([1, 2, 3], [2, 3]) == 1 and rs.distance([1, 2, 3], [1, 9, 3]) == 1


# ---------------------------------------------------------------- 2. tables and refusals
def test_table_builder_against_the_package():
    from covomix_amd import ops
    lengths = [0, 5, 0, 4096, 1, 17]
    pairs = [(0, 1), (3, 3), (5, 0), (1, 4), (0, 1)]
    items, prs = ops.edit_distance_tables(lengths, pairs)
    want_items, want_pairs = rs.tables(lengths, pairs)
    assert items.dtype == torch.int32 and prs.dtype == torch.int32 and items.is_contiguous() and prs.is_contiguous()
    assert np.array_equal(items.numpy(), want_items) and np.array_equal(prs.numpy(), want_pairs)
    assert items[:, 0].tolist() == [0, 0, 5, 5, 4101, 4102]
    items, prs = ops.edit_distance_tables([], [])
    assert items.shape == (0, 2) and prs.shape == (0, 2)
    assert ops.EDIT_MAX_LEN == rs.MAX_LEN == 4096


def test_host_layer_refusals():
    from covomix_amd import _lib, ops
    ok = [torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)]
    for lengths, pairs in (([4097], []), ([-1], []), ([3, 3], [(0, 2)]), ([3, 3], [(-1, 0)]), ([3], [(0,)]), ([3], [(0, 0, 0)]), ([3], [0]),
                           ([3], [(0, 0.0)]), ([3], [(True, 0)])):
        with pytest.raises(ValueError, match="edit_distance"):
            ops.edit_distance_tables(lengths, pairs)
    with pytest.raises(ValueError):
        ops.edit_distance([torch.zeros(4097, dtype=torch.int64)], [(0, 0)])
    for bad in ([torch.zeros(3, dtype=torch.int32)], [torch.zeros(3, 1, dtype=torch.int64)], [[1, 2, 3]]):
        with pytest.raises(TypeError):
            ops.edit_distance(bad, [(0, 0)])
    with pytest.raises(ValueError):
        ops.edit_distance(ok, [(0, 2)])
    empty = ops.edit_distance(ok, [])                                      # no pairs: no launch, so no GPU needed
    assert empty.dtype == torch.int32 and empty.shape == (0,) and empty.device.type == "cpu"
    if not torch.cuda.is_available():
        with pytest.raises(_lib.CovomixHipError):
            ops.edit_distance(ok, [(0, 1)])
        with pytest.raises(_lib.CovomixHipError):
            ops.edit_distance(ok, [(0, 1)], device="cpu")


def test_entry_point_refuses_on_the_host_copies():
    """every malformed table is refused from the host copies, before the device pointers are looked at (they are never dereferenced on the
    host, so dummies do here); n_pairs = 0 succeeds without a launch"""
    from covomix_amd import _lib
    lib = _lib.load()

    def call(items, pairs, n_tokens, n_items=None, n_pairs=None, null_items=False, null_pairs=False):
        it = np.asarray(items, dtype=np.int32).reshape(-1, 2)
        pr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        return lib.cvx_edit_distance_i64(None, n_tokens, None if null_items else it.ctypes.data, None, len(it) if n_items is None else n_items,
                                         None if null_pairs else pr.ctypes.data, None, len(pr) if n_pairs is None else n_pairs, None, None)

    good = [(0, 4), (4, 0), (4, 6)]
    assert call(good, [], 10) == 0 and call([], [], 0) == 0 and call(good, [], 10, null_pairs=True) == 0
    for what, rc in (("offset + length past the pool", call([(0, 4), (4, 7)], [(0, 1)], 10)),
                     ("negative offset", call([(-1, 4)], [(0, 0)], 10)),
                     ("negative length", call([(0, -1)], [(0, 0)], 10)),
                     ("length 4097", call([(0, 4097)], [(0, 0)], 5000)),
                     ("offset past the pool", call([(11, 0)], [(0, 0)], 10)),
                     ("pair index = n_items", call(good, [(0, 3)], 10)),
                     ("negative pair index", call(good, [(-1, 0)], 10)),
                     ("negative n_tokens", call([], [], -1)),
                     ("negative n_items", call(good, [], 10, n_items=-1)),
                     ("negative n_pairs", call(good, [(0, 1)], 10, n_pairs=-1)),
                     ("no item table", call(good, [(0, 1)], 10, null_items=True)),
                     ("no pair table", call(good, [(0, 1)], 10, null_pairs=True)),
                     ("a bad item no pair names", call([(0, 4), (4, 7)], [], 10)),
                     ("null device pointers", call(good, [(0, 1)], 10))):
        assert rc == EINVAL, what
        assert b"edit_distance" in lib.cvx_last_error_string(), what


# ---------------------------------------------------------------- 3. counted tokens
def test_counted_tokens_against_sequence_logprob():
    from covomix_amd.t2s import counted_mask, counted_tokens, sequence_logprob
    eos = 9
    streams = torch.tensor([[9, 1, 2, 3, 4, 5],          # eos first
                            [1, 2, 3, 4, 5, 9],          # eos last
                            [1, 2, 3, 4, 5, 6],          # no eos
                            [1, 9, 3, 9, 5, 6]])         # twice: the first one counts
    got = counted_tokens(streams, eos)
    assert [t.tolist() for t in got] == [[9], [1, 2, 3, 4, 5, 9], [1, 2, 3, 4, 5, 6], [1, 9]]
    assert all(t.dtype == torch.int64 and t.dim() == 1 for t in got)
    assert [t.tolist() for t in got] == [rs.counted(row.tolist(), eos) for row in streams]
    assert [t.tolist() for t in counted_tokens(streams[3], eos)] == [[1, 9]]
    # sequence_logprob averages over exactly these positions: log-probs that are 1 on them and huge elsewhere
    lp = torch.where(counted_mask(streams, eos), torch.ones(4, 6), torch.full((4, 6), 1e6))
    assert sequence_logprob(lp, streams, eos) == 1.0
    assert int(counted_mask(streams, eos).sum()) == sum(t.numel() for t in got) == 15
    for row in range(4):                                 # and stream by stream, from distinct log-probs
        lp = torch.arange(6, dtype=torch.float32) + 10 * row
        n = got[row].numel()
        assert sequence_logprob(lp[None], streams[row:row + 1], eos) == float(lp[:n].double().sum() / n)
    with pytest.raises(ValueError):
        counted_tokens(torch.zeros(2, 2, 2, dtype=torch.int64), eos)


# ---------------------------------------------------------------- 4. consensus and the token error rate
def _fake_edit_distance(calls):
    def run(sequences, pairs, device=None):
        calls.append(len(pairs))
        return torch.from_numpy(rs.distances([s.numpy() for s in sequences], pairs))
    return run


def test_consensus_differs_from_the_logprob_choice(monkeypatch):
    """three near-identical long candidates and one short outlier with the best mean log-prob: log-prob keeps the outlier, consensus a
    long one"""
    from covomix_amd import ops, t2s
    calls = []
    monkeypatch.setattr(ops, "edit_distance", _fake_edit_distance(calls))
    eos, L = 500, 24
    base = list(range(1, 21)) + [eos]

    def cand(tokens, lp):
        st = torch.tensor([tokens + [0] * (L - len(tokens))])
        return (st.reshape(-1), st, torch.full((1, L), lp))
    long0, long1, long2 = base, base[:7] + [77] + base[8:], base[:12] + [88] + base[13:]
    cands = [cand([3, eos], -0.1), cand(long0, -1.0), cand(long1, -0.9), cand(long2, -1.1)]
    scores = [t2s.sequence_logprob(c[2], c[1], eos) for c in cands]
    risks = t2s.consensus_risks(cands, eos)
    assert calls == [6]                                                       # S N (N - 1) / 2 unordered pairs, one call
    assert risks == rs.consensus_risks([c[1].tolist() for c in cands], eos)
    assert risks[1] == 1 + 1 + rs.distance([3, eos], long0) and risks[0] > max(risks[1:])
    assert t2s.best_candidate(scores) == 0 and t2s.consensus_candidate(risks, scores) == 1
    assert rs.consensus_candidate(risks, scores) == 1
    # the many-utterance form: all pairs in one call, utterances of different N, two streams
    two = [(torch.cat((c[1][0], c[1][0])), torch.cat((c[1], c[1].flip(1))), torch.cat((c[2], c[2]))) for c in cands[:3]]
    calls.clear()
    many = t2s.consensus_risks([cands, two, cands[:1]], eos)
    assert calls == [6 + 2 * 3] and many[0] == risks and many[2] == [0]
    assert many[1] == rs.consensus_risks([c[1].tolist() for c in two], eos)
    with pytest.raises(ValueError):
        t2s.consensus_risks([[]], eos)


def test_consensus_candidate_tie_rules():
    from covomix_amd.t2s import consensus_candidate
    nan = math.nan
    for risks, scores, want in (([5, 3, 3, 9], [-0.1, -2.0, -1.0, -0.5], 2),          # risk tie -> the larger score
                                ([3, 3, 3], [-1.0, -1.0, -1.0], 0),                    # then the lowest index
                                ([4, 3, 3, 3], [0.0, -1.0, -0.5, -0.5], 2),
                                ([3, 3], [nan, -7.0], 1),                              # a NaN never wins against a number
                                ([3, 3], [-7.0, nan], 0),
                                ([3, 3], [nan, nan], 0),
                                ([2, 3], [nan, 0.0], 0),                               # the risk comes first, whatever the score
                                ([7], [-1.0], 0)):
        assert consensus_candidate(risks, scores) == want == rs.consensus_candidate(risks, scores), (risks, scores)
    for bad in (([], []), ([1, 2], [0.0])):
        with pytest.raises(ValueError):
            consensus_candidate(*bad)


def test_token_error_rate_hand_cases(monkeypatch):
    from covomix_amd import ops, t2s
    calls = []
    monkeypatch.setattr(ops, "edit_distance", _fake_edit_distance(calls))
    T = lambda *v: torch.tensor(v, dtype=torch.int64)
    assert t2s.token_error_rate(T(1, 2, 3), T(1, 2, 3)) == 0.0                                   # equal
    assert t2s.token_error_rate(T(1, 2), T(1, 2, 3, 4)) == 2 / 4                                 # shorter: the pads are two substitutions
    assert t2s.token_error_rate(T(1, 2, 3, 4, 5), T(1, 2, 3)) == 2 / 5                           # longer: over the PADDED reference length
    assert t2s.token_error_rate(T(7, 1, 2, 3), T(1, 2, 3)) == 2 / 4                              # shifted: delete 7, insert the pad
    assert t2s.token_error_rate(T(), T()) == 0.0 and t2s.token_error_rate(T(), T(4, 4)) == 1.0
    assert t2s.token_error_rate(T(501), T()) == 0.0                                              # the pad value is a token like any other
    n = len(calls)
    preds, refs = [T(1, 2, 3), T(), T(1, 2), T(), T(9)], [T(1, 2, 3), T(), T(1, 2, 3, 4), T(4, 4), T(8)]
    lst = t2s.token_error_rate(preds, refs)
    assert lst == [0.0, 0.0, 0.5, 1.0, 1.0] and calls[n:] == [4]                                  # one launch; the empty pair is not in it
    assert lst == [rs.token_error_rate(p.tolist(), r.tolist()) for p, r in zip(preds, refs)]
    assert t2s.token_error_rate(T(1, 2), T(1, 2, 3), pad=3) == 0.0
    with pytest.raises(ValueError):
        t2s.token_error_rate([T(1)], [T(1), T(2)])
    with pytest.raises(ValueError):
        t2s.token_error_rate(T(1), [T(1)])


# ---------------------------------------------------------------- 5. CLI, facade, ABI
def test_cli_flag():
    from covomix_amd import generation
    p = generation.build_parser()
    kw = lambda *a: generation.t2s_sampling_kwargs(p.parse_args(list(a)))
    assert kw() == {} and kw("--t2s_best_of_select", "logprob") == {}
    assert kw("--t2s_best_of", "4", "--t2s_best_of_select", "logprob") == dict(best_of=4)
    assert kw("--t2s_best_of", "4", "--t2s_best_of_select", "mbr") == dict(best_of=4, best_of_select="mbr")
    assert kw("--t2s_best_of_temperatures", "0.7,1.0", "--t2s_best_of_select", "mbr") == \
        dict(best_of_temperatures=(0.7, 1.0), best_of_select="mbr")
    for bad in (["--t2s_best_of_select", "mbr"], ["--t2s_best_of", "1", "--t2s_best_of_select", "mbr"],
                ["--t2s_beam_size", "4", "--t2s_best_of_select", "mbr"]):
        with pytest.raises(ValueError, match="t2s_best_of_select"):
            kw(*bad)
    with pytest.raises(SystemExit):
        p.parse_args(["--t2s_best_of_select", "median"])


def test_facade_value_errors():
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel
    sig = inspect.signature(CoVoMixModel.synthesis_sample_text2semantic).parameters
    assert sig["best_of_select"].default == "logprob" and list(sig)[-1] == "best_of_select"
    shapes = syn.t2s_param_shapes(two_output=False, dim=64, dim_target=64, source_depth=2, target_depth=2, heads=1, num_text=200)
    sd = {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(shapes, seed=0).items()}
    m = CoVoMixModel(sd, hparams={"text2semantic": True}).eval()
    ids = torch.ones(1, 5, dtype=torch.int64)
    for kw in (dict(best_of_select="mbr"), dict(best_of_select="mbr", best_of=1), dict(best_of_select="median", best_of=4),
               dict(best_of_select=None, best_of=4), dict(best_of_select="mbr", best_of=4, beam_search_decode=True),
               dict(best_of_select="mbr", beam_search_decode=True)):
        with pytest.raises(ValueError, match="best_of_select"):
            m.synthesis_sample_text2semantic(ids, **kw)
    for bad in ((ids, [ids]), ([ids], ids), ([ids], [ids, ids]), ([], [])):
        with pytest.raises(ValueError, match="evaluate_text2semantic"):
            m.evaluate_text2semantic(*bad)
    with pytest.raises(ValueError, match="evaluate_text2semantic"):
        m.evaluate_text2semantic([ids], [ids[0]], return_logprobs=True)


def test_header_and_binding():
    from covomix_amd import _lib
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "covomix_hip.h")).read())
    assert "#define CVX_ABI_VERSION 113" in hdr and _lib.ABI_VERSION == 113
    assert "#define CVX_EDIT_MAX_LEN 4096" in hdr and _lib.EDIT_MAX_LEN == 4096
    assert ("int cvx_edit_distance_i64(const int64_t* tokens_dev, int64_t n_tokens, const int32_t* items_host, const int32_t* items_dev, "
            "int32_t n_items, const int32_t* pairs_host, const int32_t* pairs_dev, int32_t n_pairs, int32_t* out_dev, cvx_stream_t s);") in hdr
    res, args = _lib.SIGNATURES["cvx_edit_distance_i64"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p]
    lib = _lib.load()
    assert lib.cvx_version() == 113 and lib.cvx_edit_distance_i64
    assert os.path.isfile(os.path.join(ROOT, "neurips2024-covomix_amd", "csrc", "edit_distance.hip"))
