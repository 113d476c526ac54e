"""CPU: the fp64 oracle of the vocoder kernels' per-item lengths against itself, and the proof that the checks of
test_vocoder_items_gpu.py can fail: three deliberately wrong fp64 variants of the fused pair and of the ResBlock stage, on the very
inputs the GPU test uses, miss its checks by 100 x their bounds and more.

Which check catches which fault (n = an item's length, L the common one):
  intermediate not zeroed behind n : (d) on every item with 0 < n < L   (behind the end the output is still zeroed: (a) is blind)
  end one too far  (n + 1)         : (a) and (d) on every item with 0 < n < L
  end one too near (n - 1)         : (d) on every item with n > 0        ((a) is blind)
  accum added behind the end       : (a), on the launch whose accum breaks the input rule ((d) is blind; with an accum that obeys
                                     the rule this variant IS the correct result - which is why the GPU test has that launch)
(a)'s own bound is zero; 'by 100 x' is measured against the smallest error the kernel's accuracy bound could hide there,
100 x BOUND x max|expected|."""
import pytest
import torch

import vocoder_items_oracle as vio

BOUND = 5e-6            # the (c) bound of the pair / ResBlock kernels (test_resblock_pair_fused_kernel, test_resblock_f16x3_entry_point)
MISS = 100.0


def _tail1(got, want, n):
    return vio.rel_tails(got[None], want[None], [n])[0]


def _behind1(got, n):
    return vio.max_behind(got[None], [n])


@pytest.mark.parametrize("R,pad,L", [(256, 25, 601), (160, 1, 320), (192, 9, 384), (256, 15, 512), (118, 5, 371), (800, 6, 1001)])
def test_length_launches_cover_the_edges(R, pad, L):
    ls = vio.length_launches(R, pad, L)
    assert len(ls) <= 3 and all(len(f) <= 8 for f, _, _ in ls)
    got = set()
    for la in ls:
        got |= set(vio.lens_of(la, L))
    assert vio.required_lengths(R, pad, L) <= got, vio.required_lengths(R, pad, L) - got
    raw = [f * m + a for fr, m, a in ls for f in fr]
    assert min(raw) < 0 and max(raw) > L                        # both clamps of cvx_item_len
    assert any(m != 1 and a != 0 for _, m, a in ls)


@pytest.mark.parametrize("C,flags", vio.PAIR_INST)
@pytest.mark.parametrize("k,dil", vio.PAIR_KD)
def test_pair_checks_catch_every_fault(C, flags, k, dil):
    R, pad, L, launches = vio.pair_case(C, flags, k, dil)
    for li, la in enumerate(launches):
        lens = vio.lens_of(la, L)
        x, acc, c1, c2 = vio.pair_inputs(C, k, dil, L, lens, seed=1000 * C + 10 * k + li)
        dirty = vio.dirty_accum(acc, lens, seed=li)
        c1, c2 = vio.dbl(c1), vio.dbl(c2)
        for b, n in enumerate(lens):
            if n == 0:
                continue
            xb, ab, db = x[b].double(), acc[b].double(), dirty[b].double()
            want = torch.zeros(C, L, dtype=torch.float64)
            want[:, :n] = vio.pair_item(xb[:, :n], c1, c2, dil, ab[:, :n], 0.5)
            ok = vio.pair_padded(xb, n, c1, c2, dil, ab, 0.5)
            assert float((ok - want).abs().max()) < 1e-12       # the padded restatement IS the B = 1 run
            assert float((vio.pair_padded(xb, n, c1, c2, dil, db, 0.5) - want).abs().max()) < 1e-12
            floor = MISS * BOUND * float(want.abs().max())
            if n < L:
                v = vio.pair_padded(xb, n, c1, c2, dil, ab, 0.5, fault="t_unmasked")
                assert _tail1(v, want, n) > MISS * 4 * BOUND and _behind1(v, n) == 0.0
                v = vio.pair_padded(xb, n, c1, c2, dil, ab, 0.5, fault="len+1")
                assert _tail1(v, want, n) > MISS * 4 * BOUND and _behind1(v, n) > floor
                v = vio.pair_padded(xb, n, c1, c2, dil, db, 0.5, fault="accum_behind")
                assert _behind1(v, n) > floor and _tail1(v, want, n) < 1e-12
                assert float((vio.pair_padded(xb, n, c1, c2, dil, ab, 0.5, fault="accum_behind") - want).abs().max()) < 1e-12
            v = vio.pair_padded(xb, n, c1, c2, dil, ab, 0.5, fault="len-1")
            assert _tail1(v, want, n) > MISS * 4 * BOUND


@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_resblock_stage_checks_catch_every_fault(name):
    """the stage's inputs of the GPU test (its second launch: mul = 2, add < 0).  Wide stage: the fault sits in the k = 3 block only
    (a third of the sum, the cheapest to evaluate) - it still misses the checks by the same factor."""
    cs = vio.STAGE_CASES[name]
    C, L = cs["C"], cs["L"]
    la = vio.length_launches(cs["R"], cs["pad"], L)[1]
    lens = vio.lens_of(la, L)
    x, acc, blocks = vio.resblock_inputs(C, vio.STAGE_KS, L, lens, seed=77 + C)
    fb = None if name == "narrow" else [0]
    for b, n in enumerate(lens):
        if n == 0:
            continue
        xb = x[b].double()
        want = torch.zeros(C, L, dtype=torch.float64)
        want[:, :n] = vio.stage_item(xb[:, :n], blocks)
        good = vio.stage_padded(xb, n, blocks)
        assert float((good - want).abs().max()) < 1e-11
        floor = MISS * BOUND * float(want.abs().max())
        if n < L:
            v = vio.stage_padded(xb, n, blocks, "t_unmasked", fb)
            assert _tail1(v, want, n) > MISS * 4 * BOUND and _behind1(v, n) == 0.0
            v = vio.stage_padded(xb, n, blocks, "len+1", fb)
            assert _tail1(v, want, n) > MISS * 4 * BOUND and _behind1(v, n) > floor
        v = vio.stage_padded(xb, n, blocks, "len-1", fb)
        assert _tail1(v, want, n) > MISS * 4 * BOUND


def test_resblock_accum_behind_the_end_is_caught():
    """one narrow ResBlock (k = 7) with an accum that breaks the input rule - the GPU test's launch of the same name"""
    cs = vio.STAGE_CASES["narrow"]
    C, L = cs["C"], cs["L"]
    lens = vio.lens_of(vio.length_launches(cs["R"], cs["pad"], L)[1], L)
    x, acc, blocks = vio.resblock_inputs(C, vio.STAGE_KS, L, lens, seed=77 + C)
    dirty = vio.dirty_accum(acc, lens, seed=3)
    blk = [(vio.dbl(c1), vio.dbl(c2)) for c1, c2 in blocks[1]]
    for b, n in enumerate(lens):
        if n == 0 or n == L:
            continue
        xb, db = x[b].double(), dirty[b].double()
        want = torch.zeros(C, L, dtype=torch.float64)
        want[:, :n] = vio.resblock_item(xb[:, :n], blk, vio.RESBLOCK_DILS, db[:, :n], 1.0 / 3)
        assert float((vio.resblock_padded(xb, n, blk, vio.RESBLOCK_DILS, db, 1.0 / 3) - want).abs().max()) < 1e-11
        v = vio.resblock_padded(xb, n, blk, vio.RESBLOCK_DILS, db, 1.0 / 3, fault="accum_behind")
        assert _behind1(v, n) > MISS * BOUND * float(want.abs().max())
