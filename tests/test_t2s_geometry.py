"""CPU: the case table of tests/test_t2s_geometry_gpu.py as data.  tests/t2s_geometry.py restates the launch arithmetic of one
text2semantic token step (csrc/t2s_decode.hip); this file holds the table to it - every kernel path class the GPU file is there to
launch is reached by one of its cases and by NONE of the four fixture geometries the rest of the suite decodes with - and checks
that the fp64 oracle can tell, on exactly these models and inputs, what the GPU file asks of it:
  * the oracle restated in fp32 stays inside LONG_LOGIT_TOL at every position (so the bound is reachable by fp32 arithmetic at these
    widths, 4096 included);
  * a kernel that loses the last 4-vector of a row, the last output row or the last logit is outside it at every position;
  * the reference's choice is decidable on nearly every step (so the token check is not vacuous).
Measured (a record, not a threshold), random forced tokens: the fp32 restatement 8.1e-7 (k4096-v65) to 2.0e-6 (k4-v5) from fp64; the
smallest figure of a wrong variant over all cases and positions 5.6e-5 (ff.4's last row, k1020-h2-v1023: one of 1020 residual entries
loses its feed-forward term), 3.7 times the bound, the next 1.4e-4 (the last logit, k64-ff4095); decidable share 0.99 to 1.0."""
import pytest
import torch

import t2s_geometry as tg
import t2s_oracle as orc

TOL = orc.LONG_LOGIT_TOL
P = "target_transformer.layers.0"


def test_case_table():
    pads = {"k4-v5": (10, 12), "k260-h3-v501": (693, 696), "k1020-h2-v1023": (2720, 2720), "k1028-h1-v1024": (2741, 2744),
            "k1536-ff4096": (4096, 4096), "k4096-v65": (1001, 1004), "k64-ff4095": (4095, 4096), "two-k520-v333": (1386, 1388),
            "two-k8-v9": (21, 24)}
    assert list(pads) == list(tg.CASES)
    for name, c in tg.CASES.items():
        d = tg.dims(**c)
        assert (d["ff_inner"], d["ff_inner_pad"]) == pads[name], name
        assert tg.admitted(d), name
    assert tg.dims(**tg.CASES["two-k8-v9"])["dim_emb"] == 4 and tg.dims(**tg.CASES["two-k520-v333"])["dim_emb"] == 260
    assert tg.top_k(5) == 1 and tg.top_k(9) == 1 and tg.top_k(1024) == 103
    for name, c in tg.EXISTING.items():
        assert tg.admitted(tg.dims(**c)), name
    # what the GPU file's refusal cases change, one field each
    base = tg.dims(**tg.CASES["k260-h3-v501"])
    for change in (dict(dim=4100, dim_emb=4100), dict(ff_inner_pad=4100), dict(vocab=1025), dict(streams=2, dim=1028, dim_emb=514),
                   dict(streams=2, dim=1032, dim_emb=516)):
        assert not tg.admitted({**base, **change}), change


def test_launch_arithmetic_of_the_cases():
    """spot checks of the restatement against the figures worked out by hand from launch_gemv_b and load_chunk"""
    L = {l["name"]: l for l in tg.gemv_launches(tg.dims(**tg.CASES["k260-h3-v501"]), 9)}
    assert L["wo_s"]["pairs"] == 130 and L["wo_s"]["row_blocks"] == 33 and L["wo_s"]["idle_waves"] == 2 and L["wo_s"]["exit_blocks"] == 7
    assert L["wo_s"]["K"] == 192 and L["wo_s"]["chunks"] == ((("partial", 48), "absent", "absent", "absent"),)
    assert L["qkv_s"]["chunks"] == (("whole", ("partial", 1), "absent", "absent"),) and L["qkv_s"]["BQ"] == 8 and L["qkv_s"]["groups"] == 2
    assert L["qkv_s"]["row_blocks"] == 72 and L["wq_c"]["row_blocks"] == 24 and L["qkv_s"]["exit_blocks"] == 0
    assert L["logits"]["pairs"] == 251 and L["logits"]["no_second_row"] and L["w1"]["zero_fill"] == 3
    assert tg.gemv_launches(tg.dims(**tg.CASES["k260-h3-v501"]), 5)[1]["exit_blocks"] == 0           # one group: the grid is not padded
    assert [tg.gemv_launches(tg.dims(**tg.CASES["k4-v5"]), s)[0]["BQ"] for s in tg.SLOT_FORMS] == [1, 2, 4, 8, 8]
    L = {l["name"]: l for l in tg.gemv_launches(tg.dims(**tg.CASES["k1028-h1-v1024"]), 1)}
    assert L["w1"]["chunks"] == (("whole",) * 4, (("partial", 1), "absent", "absent", "absent"))
    assert L["w2"]["K"] == 2744 and len(L["w2"]["chunks"]) == 3 and L["w2"]["chunks"][2] == ("whole", "whole", ("partial", 46), "absent")
    L = {l["name"]: l for l in tg.gemv_launches(tg.dims(**tg.CASES["k1020-h2-v1023"]), 1)}
    assert L["wq_c"]["chunks"] == (("whole", "whole", "whole", ("partial", 63)),) and L["w1"]["zero_fill"] == 0
    L = {l["name"]: l for l in tg.gemv_launches(tg.dims(**tg.CASES["two-k520-v333"]), 1)}
    assert L["logits"]["K"] == 260 and L["logits"]["Kin"] == 520 and L["logits"]["pairs"] == 334 and len(L["logits"]["chunks"]) == 1
    L = {l["name"]: l for l in tg.gemv_launches(tg.dims(**tg.CASES["k4096-v65"]), 1)}
    assert all(L[n]["chunks"] == (("whole",) * 4,) * 4 for n in ("qkv_s", "wq_c", "w1", "logits"))
    L = {l["name"]: l for l in tg.gemv_launches(tg.dims(**tg.CASES["k1536-ff4096"]), 1)}
    assert L["w2"]["chunks"] == (("whole",) * 4,) * 4 and L["w1"]["chunks"] == (("whole",) * 4, ("whole", "whole", "absent", "absent"))


def test_every_path_class_is_reached_by_a_case_and_by_no_fixture_geometry():
    reached = {name: tg.case_paths(c) for name, c in tg.CASES.items()}
    for name, c in tg.EXISTING.items():
        assert tg.case_paths(c) == set(), (name, tg.case_paths(c))
    union = set().union(*reached.values())
    assert union == set(tg.PATHS), (set(tg.PATHS) - union, union - set(tg.PATHS))
    # what each case is in the table for
    norm = lambda k: {f"{k}:{m}" for m in tg.NORM_MODES}
    assert {"norm-one-lane-strip", "idle-waves:RES", "sample-V-below-a-wave", "logits-odd-vocab"} <= reached["k4-v5"]
    assert norm("norm-whole-then-partial-strip") | {"idle-waves:RES", "exit-blocks:RES", "logits-odd-vocab", "norm-one-lane-strip"} <= reached["k260-h3-v501"]
    assert {"norm-strip-one-lane-short", "geglu-zero-fill-0", "sample-V-1023", "logits-odd-vocab"} <= reached["k1020-h2-v1023"]
    assert norm("norm-second-chunk-one-vector") | {"sample-V-1024", "logits-multi-chunk"} <= reached["k1028-h1-v1024"]
    assert norm("norm-second-chunk") | {"geglu-ff-pad-max", "geglu-zero-fill-0"} <= reached["k1536-ff4096"]
    assert norm("norm-K-max") | norm("norm-second-chunk") | {"logits-multi-chunk"} <= reached["k4096-v65"]
    assert {"geglu-zero-fill-1", "geglu-ff-pad-max"} <= reached["k64-ff4095"]
    assert {"logits-slice-offset-unaligned", "logits-odd-vocab", "norm-whole-then-partial-strip:LOGITS"} <= reached["two-k520-v333"]
    assert {"logits-odd-vocab", "sample-V-below-a-wave"} <= reached["two-k8-v9"]
    # exiting row blocks need the padded grid: nine slots
    assert "exit-blocks:RES" not in tg.paths(tg.gemv_launches(tg.dims(**tg.CASES["k260-h3-v501"]), 5))


# ---------------------------------------------------------------- the oracle on these models
_BASE = {}


def base(name):
    """(state dict, text, forced tokens [S, L], fp64 teacher-forced logits [L, S, V]): computed once, shared, never modified"""
    if name not in _BASE:
        sd, src, streams = tg.state_dict(name), tg.text(), tg.forced_tokens(name)
        with torch.no_grad():
            _BASE[name] = (sd, src, streams, orc.teacher_forced_logits(sd, src, streams))
    return _BASE[name]


@pytest.mark.parametrize("name", list(tg.CASES))
def test_fp32_restatement_is_inside_the_bound(name):
    sd, src, streams, tf = base(name)
    with torch.no_grad():
        per = orc.per_position_rel_l2(orc.teacher_forced_logits(sd, src, streams, dtype=torch.float32), tf)
    print(f"{name}: fp32 restatement, max per-position rel-L2 {float(per.max()):.3e} (at {int(per.argmax())})")
    assert per.shape == (tg.STEPS,) and float(per.max()) <= TOL, (name, float(per.max()))


def wrong_variants(sd):
    """name -> (state dict of a decoder that a subtly wrong kernel would compute, first position it must show at)"""
    def zeroed(key, cols=None, row=None):
        w = sd[key].clone()
        if cols is not None:
            w[:, -cols:] = 0
        if row is not None:
            w[row, :] = 0
        return {**sd, key: w}
    return {"to_q self, last 4 columns": (zeroed(P + ".0.to_q.0.weight", cols=4), 1),       # (one key at position 0: q cannot matter)
            "to_q cross, last 4 columns": (zeroed(P + ".1.to_q.0.weight", cols=4), 0),
            "ff.1, last 4 columns": (zeroed(P + ".2.1.weight", cols=4), 0),
            "to_out self, last 4 columns": (zeroed(P + ".0.to_out.weight", cols=4), 0),
            "ff.4, last 4 columns": (zeroed(P + ".2.4.weight", cols=4), 0),
            "ff.4, last row": (zeroed(P + ".2.4.weight", row=-1), 0)}


@pytest.mark.parametrize("name", list(tg.CASES))
def test_oracle_resolves_a_lost_vector_row_or_logit(name):
    sd, src, streams, tf = base(name)
    worst = {}
    for what, (bad, first) in wrong_variants(sd).items():
        with torch.no_grad():
            per = orc.per_position_rel_l2(orc.teacher_forced_logits(bad, src, streams), tf)[first:]
        worst[what] = float(per.min())
    lost = tf.clone()
    lost[..., -1] = 0
    worst["last logit left at 0"] = float(orc.per_position_rel_l2(lost, tf).min())
    print(f"{name}: smallest per-position rel-L2 of the wrong variants: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for what, v in worst.items():
        assert v > TOL, (name, what, v)


def test_reference_choice_is_decidable_on_these_inputs():
    tot_dec = tot = 0
    for name, c in tg.CASES.items():
        _, _, _, tf = base(name)
        _, dec = orc.reference_choice(tf, tg.draws(tg.STEPS, c["outputs"], c["vocab"], seed=21))
        share = float(dec.double().mean())
        print(f"{name}: decidable share of the reference's choices {share:.4f}")
        assert share >= 0.9, (name, share)
        tot_dec, tot = tot_dec + int(dec.sum()), tot + dec.numel()
    assert tot_dec >= 0.98 * tot, (tot_dec, tot)
