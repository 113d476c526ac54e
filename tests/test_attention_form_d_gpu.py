"""Form D of the split-precision attention (256-query blocks, four waves with two query sets of 32 each).  Single-term
launches of the same size stay on form A1 - the single-term twin of the geometry was built and measured slower - and are run here too.

MAIN CLAIM: a query's output does not depend on whether form A or form D computed it.  One large launch (form D by the library's own
rule) is compared with torch.equal against the same sequences launched in groups that the rule gives form A (fewer than 512 blocks
of 256 queries, 2048 query rows and more) - fp32 output, split (hi, lo) output with out_scale, single-term twin, equal-length and
ragged.  In the ragged case every group starts at a multiple of 32 packed rows, so that a sequence's key tiles (aligned to 32 packed
rows) are the same in the large launch and in its group.

Then the fp64 bounds of tests/test_attention_forms_gpu.py (rel-L2 5e-6 and the per-row bound of 8 x the fp32 CPU row error; 1e-3
and 2^-11 ||V||inf single-term) on its input families at 32 sequences x 300 frames x 8 heads (512 blocks exactly), poisoned
neighbours, run-to-run identity, and both sides of the threshold (511 / 512 blocks)."""
import pytest
import torch

import attention_oracle as ao
from test_attention_forms_gpu import OUT_SCALE, Problem, _form_of       # the operand builder and bound checks of the forms test


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import covomix_amd.ops as o
    return o

pytestmark = pytest.mark.gpu


def _rows(lengths, i0, i1):
    cu = ao._cu(lengths)
    return cu[i0], cu[i1]


def _identity(ops, shape, H, groups, single, fam="randn", seed=3):
    """groups: list of (first sequence, end sequence) that partition the launch"""
    lengths = ao.lengths_of(shape)
    want = "A1" if single else "D"          # single-term launches stay on form A1 (measured faster): the comparison then
    # only pins that a large A1 launch equals its pieces
    assert _form_of(ops, shape, H, single) == want
    q, k, v = ao.family(fam, lengths, H, seed=seed)
    big = Problem(ops, shape, H, single, q, k, v)
    out, _, halves = big.run(scaled=OUT_SCALE)
    for i0, i1 in groups:
        r0, r1 = _rows(lengths, i0, i1)
        assert isinstance(shape, tuple) or r0 % 32 == 0
        sub = (i1 - i0, shape[1]) if isinstance(shape, tuple) else lengths[i0:i1]
        assert _form_of(ops, sub, H, single) == ("A1" if single else "A"), sub
        piece = Problem(ops, sub, H, single, q[r0:r1].clone(), k[r0:r1].clone(), v[r0:r1].clone())
        po, _, ph = piece.run(scaled=OUT_SCALE)
        assert torch.equal(po, out[r0:r1]), (shape, i0, "fp32 output")
        for a, b in zip(ph, halves):
            assert (a is None and b is None) or torch.equal(a, b[r0:r1]), (shape, i0, "split output")


@pytest.mark.parametrize("single", [False, True], ids=["D", "single-term"])
@pytest.mark.parametrize("T", [1000, 777, 1250])
def test_form_d_has_the_bits_of_form_a(ops, T, single):
    _identity(ops, (16, T), 16, [(0, 4), (4, 8), (8, 12), (12, 16)], single)


@pytest.mark.parametrize("single", [False, True], ids=["D", "single-term"])
def test_form_d_has_the_bits_of_form_a_at_one_block_per_group(ops, single):
    _identity(ops, (32, 256), 16, [(0, 8), (8, 16), (16, 24), (24, 32)], single, fam="late_rise")


RAGGED = [1000, 777, 650, 517, 300, 999, 901, 808, 256, 257, 1000, 535, 1000, 1000, 31, 657]


@pytest.mark.parametrize("single", [False, True], ids=["D", "single-term"])
def test_form_d_has_the_bits_of_form_a_ragged(ops, single):
    _identity(ops, RAGGED, 16, [(0, 4), (4, 8), (8, 12), (12, 16)], single, fam="late_rise")


BOUND_SHAPE, BOUND_H = (32, 300), 8          # 32 x 8 x 2 = 512 blocks


@pytest.mark.parametrize("single", [False, True], ids=["D", "single-term"])
def test_form_d_against_fp64(ops, single):
    name = "A1" if single else "D"
    assert _form_of(ops, BOUND_SHAPE, BOUND_H, single) == name
    bad = []
    for fam in ("randn", "dominant_j0", "dominant_j1", "dominant_j2", "dominant_j3", "dominant_jlast-1", "dominant_jlast", "dominant_perq", "late_rise", "near_uniform", "head_addr"):
        p = Problem(ops, BOUND_SHAPE, BOUND_H, single, *ao.family(fam, ao.lengths_of(BOUND_SHAPE), BOUND_H, seed=5))
        out, sp, halves = p.run(scaled=OUT_SCALE)
        bad += p.check(out, sp, f"{name} 32x300x8 {fam}", OUT_SCALE[2])
        out2, _, halves2 = p.run(scaled=OUT_SCALE)
        assert torch.equal(out, out2) and all(a is None or torch.equal(a, b) for a, b in zip(halves, halves2)), fam
    assert not bad, bad


@pytest.mark.parametrize("shape,H,form", [((73, 200), 7, "A"), ((64, 200), 8, "D")], ids=["511-blocks", "512-blocks"])
def test_both_sides_of_the_threshold(ops, shape, H, form):
    assert shape[0] * H * ((shape[1] + 255) // 256) == (512 if form == "D" else 511)
    assert _form_of(ops, shape, H, False) == form
    p = Problem(ops, shape, H, False, *ao.family("randn", ao.lengths_of(shape), H, seed=11))
    out, sp, _ = p.run(scaled=OUT_SCALE)
    assert not p.check(out, sp, f"{form} {shape} x {H}", OUT_SCALE[2])


POISON_LENGTHS = [45, 83, 70, 256, 1, 129, 200, 33] * 8        # 64 sequences x 8 heads x 1 block


def test_form_d_poisoned_neighbours_are_invisible(ops):
    lengths, H = POISON_LENGTHS, 8
    assert _form_of(ops, lengths, H, False) == "D"
    q, k, v = ao.family("randn", lengths, H, seed=13)
    p = Problem(ops, lengths, H, False, q, k, v)
    base, _, _ = p.run(split=None)
    assert not p.check(base, None, f"D poison-base {len(lengths)} sequences")
    cu = ao._cu(lengths)
    for i in (0, 1, 3, 4, 5, 31, 36, 62, 63):
        kp, vp = k.clone(), v.clone()
        kp[:cu[i]] = 3.0e4; vp[:cu[i]] = 3.0e4; kp[cu[i + 1]:] = -3.0e4; vp[cu[i + 1]:] = -3.0e4
        got, _, _ = Problem(ops, lengths, H, False, q, kp, vp).run(split=None)
        assert torch.equal(got[cu[i]:cu[i + 1]], base[cu[i]:cu[i + 1]]), i


@pytest.mark.parametrize("T", [777, 1250, 520])
def test_form_d_idle_waves_write_nothing_and_raise_no_flag(ops, T):
    """The last block of a sequence holds waves whose 64 queries all lie past its end (T = 777: three of four, T = 520: block 2 holds
    8 queries): they skip the tile loop's arithmetic.  Problem.run asserts that nothing lands behind the last row, that no NaN is
    left and that the saturation flag stays clear; head_addr puts a wrong row or head an integer away."""
    shape, H = (32, T), 8
    assert _form_of(ops, shape, H, False) == "D"
    p = Problem(ops, shape, H, False, *ao.family("head_addr", ao.lengths_of(shape), H, seed=17))
    out, sp, _ = p.run(scaled=OUT_SCALE)
    assert not p.check(out, sp, f"D {shape} x {H} head_addr", OUT_SCALE[2])
