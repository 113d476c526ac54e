"""CPU: the attention oracle against itself, the proof that the GPU test of the attention forms can fail, and the coverage of the
six kernel forms by its table of launches (asserted through the library's own launch rule, cvx_attention_f16x3_form).

A fault counts as caught on an input family when at least one variant of the family (the dominant key walks through six tiles)
moves BOTH figures the GPU test asserts - the rel-L2 of the whole output and the worst per-row error - past their bounds: the
GPU test runs every variant, so one failing variant fails it."""
import pytest
import torch

import attention_oracle as ao

# a packed batch whose sequences start mid-tile (0, 70, 403, 436: columns 0, 6, 19, 20 of their first tile); 33 frames at column 19
# are two tiles (fewer than three groups), 70 frames three (fewer than four)
LENGTHS, H = [70, 333, 33, 140], 2


def _groups(name):
    """the variants of one input family"""
    return [f for f in ao.FAMILIES if f == name or (name == "dominant" and f.startswith("dominant"))]


FAMILY_GROUPS = ("randn", "dominant", "late_rise", "near_uniform", "head_addr")


def _inputs(fam, single=False, seq0=0):
    q, k, v = ao.family(fam, LENGTHS, H, seed=3, seq0=seq0)
    return tuple(ao.split_dequant(t, single) for t in (q, k, v))


@pytest.mark.parametrize("KS", [1, 3, 4])
def test_keysplit_model_equals_reference(KS):
    """1 ... 13 tiles: fewer tiles than groups, not a multiple of the groups, unaligned first tile."""
    g = torch.Generator().manual_seed(KS)
    worst = 0.0
    for ntiles in range(1, 14):
        for off, T in ((0, 32 * ntiles), (0, 32 * ntiles - 13), (19, 32 * ntiles - 19 - 7), (31, 32 * (ntiles - 1) + 1)):
            if T <= 0:
                continue
            assert (off + T + 31) // 32 == ntiles
            q, k, v = (torch.randn(T, 64, generator=g, dtype=torch.float64) for _ in range(3))
            got = ao.keysplit_model(q, k, v, ao.SCALE, KS, tile0_offset=off)
            ref = ao.reference(q[None, :, None], k[None, :, None], v[None, :, None], ao.SCALE)[0, :, 0]
            worst = max(worst, float((got - ref).abs().max() / ref.abs().max()))
    print("keysplit_model vs reference, KS =", KS, worst)
    assert worst < 1e-12


@pytest.mark.parametrize("fam", ao.FAMILIES)
def test_keysplit_model_equals_reference_on_every_family(fam):
    q, k, v = _inputs(fam)
    ref = ao.reference(q, k, v, ao.SCALE, LENGTHS)
    for KS in (3, 4):
        got = ao.keysplit_batch(q, k, v, ao.SCALE, KS, LENGTHS)
        assert float(ao.row_error(got, ref, v).max()) < 1e-12


@pytest.mark.parametrize("fam", ao.FAMILIES)
def test_inputs_stay_inside_the_split_window(fam):
    """No value near the fp16 limit, no score near the mask sentinel, every normaliser in [1, T]: saturation is not what these
    inputs test.  Checked on the packed batch above and at the longest sequences of the GPU table."""
    for lengths, heads in ((LENGTHS, H), ([2500], 1), ([1025, 1023], 2), ([700, 1, 5, 33, 400], 2)):
        q, k, v = ao.family(fam, lengths, heads, seed=1)
        ao.check_in_window(q, k, v, ao.SCALE, lengths)


@pytest.mark.parametrize("group", FAMILY_GROUPS)
@pytest.mark.parametrize("fault", ao.FAULTS)
def test_every_fault_moves_every_family_past_the_bounds(fault, group):
    """The bounds are the ones tests/test_attention_forms_gpu.py asserts: rel-L2 5e-6 and the fp32-derived per-row bound for the
    split-precision kernels; 1e-3 and 2^-11 ||V||inf for the single-term ones."""
    for single in (False, True):
        for KS in (3, 4):
            caught = []
            for fam in _groups(group):
                # head_addr: sequence numbers 6 .. 9, constants up to 16 * 9 + 1 = 145 (a larger constant dilutes a fault more: the
                # many-tile rows of the GPU table stay below 16 * 7 + 1)
                q, k, v = _inputs(fam, single, seq0=6 if fam == "head_addr" else 0)
                ref = ao.reference(q, k, v, ao.SCALE, LENGTHS)
                bad = ao.keysplit_batch(q, k, v, ao.SCALE, KS, LENGTHS, fault=fault)
                e_tensor = ao.rel_l2(bad, ref)
                if single:
                    e_row, b_row, b_tensor = float((bad - ref).abs().max()), ao.row_bound_single_term(v), ao.F16_TOL
                else:
                    e_row, b_row, b_tensor = float(ao.row_error(bad, ref, v).max()), ao.row_bound(q, k, v, ao.SCALE, LENGTHS, ref), ao.TOL_F16X3
                print(f"{fault:20s} {fam:16s} KS={KS} single={single}: rel-L2 {e_tensor:.2e} (bound {b_tensor:.0e}), row {e_row:.2e} (bound {b_row:.2e})")
                caught.append(e_tensor > b_tensor and e_row > b_row)
            if single and group == "head_addr" and fault != "empty_group_garbage":
                # fp16 operands resolve constants of 100 and more to 2^-11 * 100 = 0.05, as much as the whole key-dependent part
                # of this family's V (0.5 / sqrt(T)): no bound the single-term kernels can meet sees a fault in the softmax WEIGHTS
                # here.  For them the family tests addressing only (next test); their merge code is the split kernels' (the
                # template parameter NT selects the number of products and nothing else), which the other four families cover.
                continue
            assert any(caught), (fault, group, KS, single)


@pytest.mark.parametrize("single", [False, True])
def test_head_addr_catches_a_wrong_head_or_sequence(single):
    q, k, v = _inputs("head_addr", single, seq0=6)
    ref = ao.reference(q, k, v, ao.SCALE, LENGTHS)
    cu = ao._cu(LENGTHS)
    wrong_head = ref.flip(1)                                           # every block wrote the other head's result
    wrong_seq = ref.clone(); wrong_seq[cu[2]:cu[3]] = ref[cu[1]:cu[1] + LENGTHS[2]]
    wrong_rows = ref.clone(); wrong_rows[..., :16] = ref[..., 16:32]  # one V^T row group for another
    for bad in (wrong_head, wrong_seq, wrong_rows):
        if single:
            assert ao.rel_l2(bad, ref) > ao.F16_TOL and float((bad - ref).abs().max()) > ao.row_bound_single_term(v)
        else:
            assert ao.rel_l2(bad, ref) > ao.TOL_F16X3 and float(ao.row_error(bad, ref, v).max()) > ao.row_bound(q, k, v, ao.SCALE, LENGTHS, ref)


def test_neighbour_leak_breaks_the_poison_identity():
    """Family 6 of the GPU test: K and V of the other sequences replaced by +-3.0e4.  The model without fault never reads them (bit
    identity holds by construction); with the mask off by one key the result moves."""
    q, k, v = _inputs("randn")
    cu = ao._cu(LENGTHS)
    kp, vp = k.clone(), v.clone()
    kp[:cu[1]] = 3.0e4; vp[:cu[1]] = 3.0e4; kp[cu[2]:] = -3.0e4; vp[cu[2]:] = -3.0e4
    for KS in (1, 3, 4):
        a = ao.keysplit_batch(q, k, v, ao.SCALE, KS, LENGTHS)[cu[1]:cu[2]]
        b = ao.keysplit_batch(q, kp, vp, ao.SCALE, KS, LENGTHS)[cu[1]:cu[2]]
        assert torch.equal(a, b)
        c = ao.keysplit_batch(q, kp, vp, ao.SCALE, KS, LENGTHS, fault="neighbour_leak")[cu[1]:cu[2]]
        assert not torch.equal(a, c) and float((a - c).abs().max()) > 1.0


def _form(shape, heads, single=False):
    from covomix_amd import ops
    if isinstance(shape, list):
        return ops.attention_form(H=heads, ragged=shape, single_term=single)
    return ops.attention_form(shape[0], shape[1], heads, single_term=single)


def test_table_of_launches_covers_every_form():
    """Every row of the GPU test's table takes the form it names (the library's own rule decides), every form appears - A, B, C at
    least twice, the single-term twins at least once - and the geometry of each form is what the kernel is instantiated with."""
    geometry = {"A": (128, 1, 4), "B": (128, 3, 4), "C": (64, 4, 2)}
    count = {}
    for row in ao.SHAPES:
        name, qb, ks, nw = _form(row["shape"], row["H"], row["single"])
        assert name == row["form"], (row["id"], name)
        assert (qb, ks, nw) == geometry[name[0]] and name.endswith("1") == row["single"], (row["id"], name, qb, ks, nw)
        count[name] = count.get(name, 0) + 1
    print(count)
    assert all(count.get(f, 0) >= 2 for f in "ABC") and all(count.get(f, 0) >= 1 for f in ("A1", "B1", "C1")), count
    ids = [r["id"] for r in ao.SHAPES]
    assert len(set(ids)) == len(ids)
    for f in "ABC":
        shape, heads = ao.VARIANT_SHAPES[f]
        assert _form(shape, heads)[0] == f
    for f, bt in ao.AGREEMENT["batches"].items():
        assert _form((bt, ao.AGREEMENT["T"]), ao.AGREEMENT["H"])[0] == f


def test_thresholds_of_the_launch_rule():
    """127 / 128 frames, 2047 / 2048 query rows (ragged with those exact totals, and 15 x 136 against 16 x 128), 128 / 160 blocks."""
    for lo, hi in ao.THRESHOLDS:
        for shape, heads, form in (lo, hi):
            assert _form(shape, heads)[0] == form, (shape, heads, form)
            assert _form(shape, heads, True)[0] == form + "1"
    (a, _, _), (b, _, _) = ao.THRESHOLDS[2]
    assert sum(a) == 2047 and sum(b) == 2048 and max(a) >= 128
    in_table = {(tuple(r["shape"]), r["H"]) for r in ao.SHAPES if not r["single"]}
    for pair in ao.THRESHOLDS:
        for shape, heads, _ in pair:
            assert (tuple(shape), heads) in in_table, shape            # each side of each threshold also RUNS on the GPU


def test_attention_form_rejects_what_no_launch_has():
    from covomix_amd import ops
    for bad in ((0, 100, 1), (1, 0, 1), (1, 100, 0)):
        with pytest.raises(ValueError):
            ops.attention_form(*bad)
