"""GPU: the edit-distance kernel (ops.edit_distance over cvx_edit_distance_i64, csrc/edit_distance.hip) against the numpy restatement
(edit_distance_restated.py), and consensus best-of-N / evaluate_text2semantic end to end on the committed cosingle_small / comix_small
models.  Every comparison is integer or bit equality."""
import numpy as np
import pytest
import torch

import edit_distance_restated as rs
from test_t2s_filters import load_small
from test_t2s_logprobs_gpu import _texts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -22
FILL = 0x5A5A5A5A
# the issue's lengths; 512 / 513 and 2049 are where the kernel changes its rows per thread (256 K: 256 / 257, 1024 / 1025, 2048 are in)
LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 4095, 4096]
EDGES = (0, 1, 4095, 4096)
MORE_LENGTHS = [511, 512, 513, 2047, 2049]


def _i64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64).reshape(-1))


def _check(seqs, pairs, device_side=False):
    from covomix_amd import ops
    got = ops.edit_distance([_i64(s).to(DEV) if device_side else _i64(s) for s in seqs], pairs)
    want = torch.from_numpy(rs.distances(seqs, pairs))
    assert got.dtype == torch.int32 and got.device.type == "cpu" and got.shape == (len(pairs),)
    assert torch.equal(got, want), [(p, int(g), int(w)) for p, g, w in zip(pairs, got, want) if g != w][:8]
    return got


def _long_short(pairs, lengths):
    """long and short blocks as neighbours: the costliest pair, the cheapest, the second costliest, ..."""
    order = sorted(pairs, key=lambda p: lengths[p[0]] * lengths[p[1]] + lengths[p[0]] + lengths[p[1]])
    out = []
    while order:
        out.append(order.pop())
        if order:
            out.append(order.pop(0))
    return out


def test_length_edges_in_one_call():
    """every length against 0, 1, 4095 and 4096 and against its neighbour in the list, over a 4-symbol alphabet"""
    rng = np.random.RandomState(0)
    seqs = [rng.randint(0, 4, size=n) for n in LENGTHS]
    pairs = [(i, j) for i in range(len(LENGTHS)) for j in range(i, len(LENGTHS))
             if LENGTHS[i] in EDGES or LENGTHS[j] in EDGES or j == i + 1]
    pairs = _long_short(pairs, LENGTHS)
    assert 55 <= len(pairs) <= 70 and LENGTHS[pairs[0][0]] * LENGTHS[pairs[1][0]] == 0
    got = _check(seqs, pairs)
    print("FIGURE distances at the length edges:", sorted(set((LENGTHS[i], LENGTHS[j], int(d)) for (i, j), d in zip(pairs, got)))[-6:])


def test_lengths_where_the_rows_per_thread_change():
    rng = np.random.RandomState(1)
    lens = MORE_LENGTHS + [256, 257, 1024, 1025, 2048]
    seqs = [rng.randint(0, 3, size=n) for n in lens]
    pairs = [(i, i) for i in range(len(lens))] + [(i, (i + 1) % len(lens)) for i in range(len(lens))]
    seqs += [s.copy() for s in seqs[:len(lens)]]                 # equal length, other tokens: (i, i + n) is no (i, i)
    for s in seqs[len(lens):]:
        s[::7] = 2 - s[::7]
    pairs += [(i, i + len(lens)) for i in range(len(lens))]
    _check(seqs, _long_short(pairs, [len(s) for s in seqs]))


def test_constructed_distances():
    rng = np.random.RandomState(2)
    n = 1000
    base = rng.permutation(n) + 1                                # all distinct
    seqs, pairs, want = [base], [], []
    for k in (0, 1, 7, 300, n):
        sub = base.copy()
        at = rng.choice(n, size=k, replace=False)
        sub[at] = 100000 + np.arange(k)                          # a disjoint alphabet
        dele = np.delete(base, rng.choice(n, size=k, replace=False))
        seqs += [sub, dele]
        pairs += [(0, len(seqs) - 2), (len(seqs) - 1, 0)]
        want += [k, k]
    for m in (2, 3, 64, 257, 999, 1000):                         # a reversal keeps at most one token in place: the middle one of an odd length
        seqs += [base[:m], base[:m][::-1].copy()]
        pairs.append((len(seqs) - 2, len(seqs) - 1))
        want.append(m - m % 2)
    got = _check(seqs, pairs)
    assert got.tolist() == want


def test_two_symbols_and_the_501_vocabulary_with_int64_values():
    rng = np.random.RandomState(3)
    lens = [600, 571, 400, 33, 600, 1200]
    two = [rng.randint(0, 2, size=n) for n in lens]
    voc = [rng.randint(0, 501, size=n) for n in lens]
    voc[4] = voc[0].copy()
    voc[4][rng.choice(600, size=40, replace=False)] = 500
    wide = [v.astype(np.int64) + (1 << 31) - 250 for v in voc]   # int64 values on both sides of 2^31 that differ in their low words
    pairs = [(i, j) for i in range(len(lens)) for j in range(i + 1, len(lens))]
    a = _check(two, pairs)
    b = _check(voc, pairs, device_side=True)
    assert int(a.max()) < int(b.max())
    from covomix_amd import ops
    c = ops.edit_distance([_i64(w).to(DEV) for w in wide], pairs)
    assert torch.equal(b, c)
    with pytest.raises(ValueError, match="int32"):                # host sequences are checked before the upload
        ops.edit_distance([_i64(w) for w in wide], pairs)


def test_repeats_same_item_and_place_in_the_table():
    rng = np.random.RandomState(4)
    seqs = [rng.randint(0, 4, size=n) for n in (700, 650, 30, 0, 1300)]
    mid = [(0, 2), (2, 4), (1, 1), (3, 4), (4, 1), (3, 3), (2, 2), (0, 4)]
    pairs = [(0, 1)] + mid[:4] + [(0, 1)] + mid[4:] + [(0, 1)]
    got = _check(seqs, pairs)
    assert got[0] == got[5] == got[-1] and got[0] > 0
    assert [int(got[k]) for k, p in enumerate(pairs) if p[0] == p[1]] == [0, 0, 0]
    assert int(got[pairs.index((3, 4))]) == 1300
    rev = _check(seqs, [(j, i) for i, j in reversed(pairs)])     # the table turned round, every pair swapped
    assert torch.equal(rev, got.flip(0))


def _raw(lib, tokens_dev, n_tokens, items, pairs, out, items_dev=None, pairs_dev=None):
    from covomix_amd import ops
    it = torch.tensor(items, dtype=torch.int32).reshape(-1, 2)
    pr = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2)
    it_d = (it if items_dev is None else torch.tensor(items_dev, dtype=torch.int32).reshape(-1, 2)).to(DEV)
    pr_d = (pr if pairs_dev is None else torch.tensor(pairs_dev, dtype=torch.int32).reshape(-1, 2)).to(DEV)
    rc = lib.cvx_edit_distance_i64(tokens_dev.data_ptr(), n_tokens, it.data_ptr(), it_d.data_ptr(), it.shape[0], pr.data_ptr(), pr_d.data_ptr(),
                                   pr.shape[0], out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    return rc


def test_nothing_behind_a_length_is_read():
    """items back to back in a pool that is followed by a poison region; the same pairs with every item in a pool of its own"""
    from covomix_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.RandomState(5)
    lens = [300, 0, 257, 64, 1, 700]
    seqs = [rng.randint(0, 3, size=n) for n in lens]
    pairs = [(i, j) for i in range(len(lens)) for j in range(len(lens))]
    alone = torch.cat([ops.edit_distance([_i64(seqs[i]), _i64(seqs[j])], [(0, 1)]) for i, j in pairs])
    assert torch.equal(alone, torch.from_numpy(rs.distances(seqs, pairs)))
    items, _ = rs.tables(lens, pairs)
    n_tok = sum(lens)
    results = []
    for poison in (0, 1, 2):                                     # every symbol of the alphabet as the poison
        pool = torch.cat([_i64(s) for s in seqs] + [torch.full((5000,), poison, dtype=torch.int64)]).to(DEV)
        out = torch.full((len(pairs),), FILL, dtype=torch.int32, device=DEV)
        assert _raw(lib, pool, n_tok, items.tolist(), pairs, out) == 0
        results.append(out.cpu())
    assert all(torch.equal(r, alone) for r in results)


def test_refusals_leave_the_output_untouched():
    from covomix_amd import _lib, ops
    lib = _lib.load()
    pool = torch.arange(5000, dtype=torch.int64, device=DEV)
    good = [(0, 4), (4, 0), (4, 6), (10, 4096)]
    out = torch.full((4,), FILL, dtype=torch.int32, device=DEV)
    fill = out.clone()
    for what, items, pairs, n_tok in (("length 4097", [(0, 4097)], [(0, 0)], 5000),
                                      ("offset + length past the pool", [(0, 4), (4, 7)], [(0, 1)], 10),
                                      ("negative offset", [(-1, 4)], [(0, 0)], 10),
                                      ("negative length", [(0, -1)], [(0, 0)], 10),
                                      ("pair index = n_items", good, [(0, 1), (0, 4)], 5000),
                                      ("negative pair index", good, [(0, 1), (-1, 0)], 5000),
                                      ("a bad item no pair names", good + [(4999, 2)], [(0, 1)], 5000),
                                      ("negative n_tokens", good[:3], [(0, 1)], -1)):
        assert _raw(lib, pool, n_tok, items, pairs, out) == EINVAL, what
        assert b"edit_distance" in lib.cvx_last_error_string() and torch.equal(out, fill), what
    with pytest.raises(ValueError):
        ops.edit_distance([torch.zeros(4097, dtype=torch.int64)], [(0, 0)])
    # no pairs: success, nothing written; then the same tables with pairs: written
    assert _raw(lib, pool, 5000, good, [], out) == 0 and torch.equal(out, fill)
    assert ops.edit_distance([torch.zeros(3, dtype=torch.int64)], []).shape == (0,)
    assert _raw(lib, pool, 5000, good, [(0, 1), (0, 2), (3, 3), (2, 3)], out) == 0
    assert out.tolist() == [4, 6, 0, 4096]                                   # disjoint tokens: the longer length
    # a device copy that is not the host copy: the block reads no token and stores -1; its neighbours are not touched by that
    out.copy_(fill)
    assert _raw(lib, pool, 5000, good, [(0, 1), (0, 2), (3, 3), (2, 3)], out, pairs_dev=[(0, 1), (0, 4), (3, 3), (-1, 3)]) == 0
    assert out.tolist() == [4, -1, 0, -1]
    assert _raw(lib, pool, 5000, good, [(0, 1), (0, 2), (3, 3), (2, 3)], out, items_dev=[(0, 4), (4, 0), (4998, 6), (10, 4097)]) == 0
    assert out.tolist() == [4, -1, -1, -1]


# ---------------------------------------------------------------- end to end
N, STEPS = 4, 24


@pytest.fixture(scope="module", params=["cosingle_small", "comix_small"])
def small(request):
    """(model, texts, uniforms [N, steps, S, V] per text, eos, the N candidates of every text from one plain generate_many call)"""
    from covomix_amd.conditional_model import CoVoMixModel
    g, sd = load_small(request.param)
    m = CoVoMixModel(sd, hparams={"text2semantic": True}).eval().to(DEV)
    S, V = g["uniforms"].shape[1], g["uniforms"].shape[-1]
    ids = _texts(g, 3, seed=11)
    gen = torch.Generator().manual_seed(13)
    us = [torch.rand(N, STEPS, S, V, generator=gen).clamp_(1e-6, 1 - 1e-6) for _ in ids]
    res = m._get_t2s().generate_many([i for i in ids for _ in range(N)], [u[c] for u in us for c in range(N)], STEPS, return_logprobs=True)
    cands = [res[j * N:(j + 1) * N] for j in range(len(ids))]
    assert S == (2 if request.param == "comix_small" else 1) and all(c[1].shape[0] == S for c in res)
    return m, ids, us, V - 1, cands


def _restated_choice(cand, eos):
    from covomix_amd.t2s import sequence_logprob
    risks = rs.consensus_risks([c[1].tolist() for c in cand], eos)
    scores = [sequence_logprob(c[2], c[1], eos) for c in cand]
    return rs.consensus_candidate(risks, scores), risks, scores


def test_mbr_returns_the_restated_choice(small, monkeypatch):
    from covomix_amd import ops
    m, ids, us, eos, cands = small
    real, calls = ops.edit_distance, []
    monkeypatch.setattr(ops, "edit_distance", lambda s, p, **kw: calls.append(len(p)) or real(s, p, **kw))
    kw = dict(max_length=STEPS, best_of=N)
    S = cands[0][0][1].shape[0]
    picks = []
    for j, (i_, u_) in enumerate(zip(ids, us)):
        c, risks, scores = _restated_choice(cands[j], eos)
        picks.append(c)
        print(f"FIGURE utterance {j}: risks {risks}, scores {[round(x, 4) for x in scores]}, consensus keeps {c}, "
              f"log-prob keeps {rs.best_candidate(scores)}")
        assert len(set(risks)) > 1, "the candidates do not differ"
        calls.clear()
        got = m.synthesis_sample_text2semantic(i_, uniforms=u_, best_of_select="mbr", **kw)
        assert calls == [S * N * (N - 1) // 2]
        assert torch.equal(got.cpu(), cands[j][c][0])
        full = m.synthesis_sample_text2semantic(i_, uniforms=u_, best_of_select="mbr", return_logprobs=True, **kw)
        assert len(full) == 3 and all(torch.equal(a.cpu(), b) for a, b in zip(full, cands[j][c]))
        score = m.score_text2semantic(i_, full[1])
        assert torch.equal(score.cpu(), full[2].cpu())                       # bit-identical to score_many of the returned tokens
    # a list of utterances: one edit-distance call for all of them, every utterance what it gets alone
    calls.clear()
    both = m.synthesis_sample_text2semantic(ids, uniforms=us, best_of_select="mbr", slots=4, **kw)
    assert calls == [len(ids) * S * N * (N - 1) // 2]
    assert all(torch.equal(b.cpu(), cands[j][picks[j]][0]) for j, b in enumerate(both))
    # candidates at their own temperatures take the same selection
    calls.clear()
    temps = m.synthesis_sample_text2semantic(ids[0], uniforms=us[0], best_of_temperatures=[1.0] * N, best_of_select="mbr", max_length=STEPS)
    assert calls == [S * N * (N - 1) // 2] and torch.equal(temps.cpu(), cands[0][picks[0]][0])


def test_logprob_selection_is_the_default_and_makes_no_edit_distance_call(small, monkeypatch):
    from covomix_amd import ops
    m, ids, us, eos, cands = small
    calls = []
    monkeypatch.setattr(ops, "edit_distance", lambda *a, **kw: calls.append(1) or (_ for _ in ()).throw(AssertionError("called")))
    kw = dict(max_length=STEPS, best_of=N)
    for j, (i_, u_) in enumerate(zip(ids, us)):
        default = m.synthesis_sample_text2semantic(i_, uniforms=u_, **kw)
        named = m.synthesis_sample_text2semantic(i_, uniforms=u_, best_of_select="logprob", **kw)
        scores = _restated_choice(cands[j], eos)[2]
        assert torch.equal(default, named) and torch.equal(default.cpu(), cands[j][rs.best_candidate(scores)][0])
    lst = m.synthesis_sample_text2semantic(ids, uniforms=us, best_of_select="logprob", return_logprobs=True, **kw)
    dft = m.synthesis_sample_text2semantic(ids, uniforms=us, return_logprobs=True, **kw)
    assert all(torch.equal(a, b) for x, y in zip(lst, dft) for a, b in zip(x, y)) and not calls


def test_evaluate_text2semantic_is_the_restated_metric(small, monkeypatch):
    from covomix_amd import ops
    m, ids, us, eos, cands = small
    real, calls = ops.edit_distance, []
    monkeypatch.setattr(ops, "edit_distance", lambda s, p, **kw: calls.append(len(p)) or real(s, p, **kw))
    S = cands[0][0][1].shape[0]
    u0 = [u[0] for u in us]
    rng = np.random.RandomState(6)
    gts = [torch.from_numpy(rng.randint(0, eos, size=n).astype(np.int64)) for n in (10, STEPS, 40)]
    flat = [cands[j][0][0] for j in range(len(ids))]              # candidate 0 = the plain decode with those uniforms
    gts[1] = flat[1][:flat[1].shape[0] // S].clone()              # one prediction that is nearly right
    gts[1][0] = (gts[1][0] + 1) % eos
    acc, wer = m.evaluate_text2semantic(ids, gts, uniforms=u0, max_length=STEPS)
    preds = [f[:f.shape[0] // 2] if S == 2 else f for f in flat]
    rates = [rs.token_error_rate(p.tolist(), g.tolist()) for p, g in zip(preds, gts)]
    print("FIGURE token error rates", rates)
    assert acc == 0.0 and isinstance(acc, float) and isinstance(wer, float) and calls == [3]
    assert wer == float(torch.tensor(rates, dtype=torch.float64).mean())
    assert 0.0 < rates[1] <= 1 / len(gts[1]) + 1e-12 and all(0.0 <= r <= 1.0 for r in rates)
    if S == 2:                                                     # the first half only: the whole flat result gives another number
        whole = [rs.token_error_rate(f.tolist(), g.tolist()) for f, g in zip(flat, gts)]
        assert whole != rates
