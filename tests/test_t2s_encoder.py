"""CPU: what tests/test_t2s_encoder_gpu.py holds the text2semantic encoder (TextToSemanticDecoder.encode_many) and its context records
(_contexts / _guided_contexts) against - the cases, packings, fp64 expectations and bounds of tests/t2s_encoder_restated.py - checked
without a GPU:

  1. the bounds come from the reference alone and cannot silently grow: the fp32 CPU oracle's distance from the fp64 one (per text, per
     row; encoder rows and context rows) stays under 1e-5 in every case and packing, and the plain-torch restatement of encode_many
     the mutants are made from agrees with the oracle to fp64 rounding;
  2. resolving power at the EDGES packing, per case: the restatement with one defect, in fp64, against the fp64 expectation.
       (a) leak     the last key of the preceding text visible to a text's queries
       (b) eos      the eos row embedded with the neighbouring id
       (c) late     the rotary angle of one row per text taken one position late
       (e) scatter  context rows one row late, the null row at index 1
     each exceed the per-row bound at least 10x in at least one row of EVERY text they touch ((a): all but the first - and, at source
     depth 1, but the eos-only text, whose two keys then carry the same value row; (b), (e): all; (c): texts of two rows and more);
     the texts a mutant does not touch come out exactly as expected.
       (d) packed   rotary tables taken at the packed row index
     is measured at the last text of MANY, where the packed index is largest: RoPE is relative, the defect only costs fp32 precision of
     the angles.  The per-row bound resolves it there (asserted; MEASURED has the figures);
  3. MANY changes the form of at least one encoder GEMM against EDGES (d260-h3, d512-h8), no row count up to 4096 does so for the case
     listed in MANY_UNREACHABLE, and EDGES and EDGES_REVERSED have the same M.

MEASURED (CPU) - a record, not a threshold.  Reference alone (fp32 CPU oracle against fp64; the bounds are 4x these; they move with the
CPU's GEMM - on the MI355X host the per-row figures were 1.08e-6 to 1.97e-6):
    case            packing  per text   per row    context per text  context per row
    cosingle_small  EDGES    8.225e-07  1.942e-06  8.480e-07         1.950e-06
    d260-h3         EDGES    9.291e-07  1.620e-06  9.831e-07         1.649e-06
    d260-h3         MANY     9.766e-07  1.502e-06  1.035e-06         1.572e-06
    d512-h8         EDGES    9.433e-07  1.269e-06  9.873e-07         1.296e-06
    d512-h8         MANY     9.668e-07  1.378e-06  1.006e-06         1.355e-06
Mutants at EDGES: the smallest, over the touched texts, of (largest per-row deviation / bound_row), and the pooled rel-L2 over all rows
(the measure of the older encoder check, whose bound is 1e-4 - it never saw a packed batch):
    case            leak              eos               late              scatter
    cosingle_small  2.3e+04  1.0e-01  1.2e+05  2.2e-01  1.2e+04  3.7e-02  1.7e+05  1.3e+00
    d260-h3         3.0e+04  6.5e-02  1.6e+05  1.6e-01  1.7e+04  2.3e-02  2.1e+05  1.2e+00
    d512-h8         3.7e+04  7.8e-02  2.2e+05  1.7e-01  2.6e+04  2.7e-02  2.7e+05  1.2e+00
(d) packed, last text of MANY: d260-h3 (first packed row 2937) largest per-row deviation 3.9e-05 against bound_row 6.0e-06, pooled 1.2e-05;
d512-h8 (row 1386) 2.4e-05 against 5.5e-06, pooled 5.8e-06.  The per-row bound RESOLVES it, by 4 - 7x; the pooled measure at 1e-4 would
not.  On the MI355X, encode_many with that defect put in by hand (not committed) missed the fp64 bounds in every packing, but by 1.02 -
1.4x only - the kernels' own rounding sits inside the same bound - while the GPU file's bit-equality checks (a text at two offsets, a
text alone against its packed rows) failed in every case: those are what catches it whatever its size.
"""
import pytest
import torch

import t2s_encoder_restated as er
import t2s_oracle as orc

SENTINEL = 12345.0
NAMES = list(er.CASES)
REACHABLE = [n for n in NAMES if n not in er.MANY_UNREACHABLE]


def null_rows(name):
    """the null key / value row [2 inner] of every decoder layer, as t2s.py packs it"""
    sd, d = er.state_dict(name), orc.t2s_dims(er.state_dict(name))
    out = []
    for i in range(d["target_depth"]):
        nkv = sd[f"target_transformer.layers.{i}.1.null_kv"]
        out.append(torch.cat((nkv[0].reshape(-1), nkv[1].reshape(-1))))
    return out


# ---------------------------------------------------------------- 1. the reference alone
@pytest.mark.parametrize("name", NAMES)
def test_reference_alone_stays_small(name):
    for packing in ("EDGES", "MANY"):
        if packing == "MANY" and name in er.MANY_UNREACHABLE:
            continue
        b = er.bounds(name, packing)
        print(f"{name} {packing}: fp32 oracle against fp64: per text {b['ref_text']:.3e}, per row {b['ref_row']:.3e}; "
              f"context rows per text {b['ctx_ref_text']:.3e}, per row {b['ctx_ref_row']:.3e}")
        for k in ("ref_text", "ref_row", "ctx_ref_text", "ctx_ref_row"):
            assert 0 < b[k] < er.REFERENCE_ALONE_MAX, (name, packing, k, b[k])
        e64, e32 = er.expectation(name, packing)
        for a, r in zip(e32, e64):                          # (trivially: the oracle inside 4x its own distance)
            assert er.per_text(a, r) <= b["bound_text"] and er.per_row(a, r) <= b["bound_row"]
        assert [e.shape[0] for e in e64] == [t + 1 for t in er.token_counts(name, packing)]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_oracle(name):
    """what the mutants are made from: encode_many restated on the packed batch == the oracle's one text per call, to fp64 rounding - in
    both orders - and the restated scatter passes the record check exactly"""
    for packing in ("EDGES", "EDGES_REVERSED"):
        e64, _ = er.expectation(name, packing)
        with torch.no_grad():
            got = er.restated_encode_many(er.state_dict(name), er.texts(name, packing))
        for a, r in zip(got, e64):
            assert a.shape == r.shape and er.per_row(a, r) < 1e-12, (name, packing, er.per_row(a, r))
    records = [15, 3, 9, 0, 12, 7, 1, 13, 5, 10]
    e64, _ = er.expectation(name, "EDGES")
    for W, null in zip(er.kv_weights(name), null_rows(name)):
        kv = er.restated_contexts(e64, W, null, records, 16, SENTINEL)
        res = er.check_records(kv, W, null, records, e64, SENTINEL)
        assert res["null_exact"] and res["untouched"] and res["row"] < 1e-12
        assert res["last"] == [e.shape[0] for e in e64] and res["last"][-1] == er.MAX_SOURCE - 1


# ---------------------------------------------------------------- 2. resolving power
@pytest.mark.parametrize("name", NAMES)
def test_mutants_exceed_the_row_bound_in_every_text_they_touch(name):
    sd, txt = er.state_dict(name), er.texts(name, "EDGES")
    e64, _ = er.expectation(name, "EDGES")
    b = er.bounds(name, "EDGES")
    # (a) at source depth 1 leaves a text of one row exactly alone: the leaked key is the preceding text's eos row, whose first-layer value
    # equals that of the text's own eos row, so the softmax weights move and their product with the values does not
    deep = orc.t2s_dims(sd)["source_depth"] >= 2
    touched = dict(leak=lambda i, rows: i > 0 and (rows >= 2 or deep), eos=lambda i, rows: True, late=lambda i, rows: rows >= 2)
    for mutant in ("leak", "eos", "late"):
        with torch.no_grad():
            got = er.restated_encode_many(sd, txt, mutant=mutant)
        worst = [float(er.row_errors(a, r).max()) for a, r in zip(got, e64)]
        ratios = [w / b["bound_row"] for i, (w, r) in enumerate(zip(worst, e64)) if touched[mutant](i, r.shape[0])]
        print(f"{name} {mutant}: smallest (largest per-row deviation / bound_row) over the {len(ratios)} touched texts {min(ratios):.3e}; "
              f"pooled over all rows {er.pooled(got, e64):.3e} (the older bound: 1e-4)")
        assert min(ratios) >= 10, (name, mutant, ratios)
        for i, (w, r) in enumerate(zip(worst, e64)):        # (and the texts a mutant does not touch are left exactly alone)
            if not touched[mutant](i, r.shape[0]):
                assert w < 1e-12, (name, mutant, i, w)
    records = list(range(len(e64)))
    for layer, (W, null) in enumerate(zip(er.kv_weights(name), null_rows(name))):
        kv = er.restated_contexts(e64, W, null, records, len(e64), SENTINEL, mutant="scatter")
        res = er.check_records(kv, W, null, records, e64, SENTINEL)
        ratios = [float(r.max()) / b["ctx_bound_row"] for r in res["rows"]]
        want = [e @ W.double().T for e in e64]
        print(f"{name} scatter, layer {layer}: smallest (largest per-row deviation / ctx_bound_row) over the {len(ratios)} texts "
              f"{min(ratios):.3e}; pooled over all rows {er.pooled([kv[r, 1:e.shape[0] + 1] for r, e in zip(records, e64)], want):.3e}")
        assert min(ratios) >= 10, (name, layer, ratios)
        assert not res["null_exact"] and not res["untouched"] and res["last"] == [e.shape[0] + 1 for e in e64]


@pytest.mark.parametrize("name", REACHABLE)
def test_packed_rotary_index_at_the_last_text_of_many(name):
    """(d): how much of the defect the fp64 bound sees - it resolves it at the last text of MANY (the module docstring has the figures).
    What catches it whatever its size is the GPU file's reordering check - a text's rows are bit-equal at two offsets - which this
    restatement fails too: asserted here."""
    sd, txt = er.state_dict(name), er.texts(name, "MANY")
    e64, _ = er.expectation(name, "MANY")
    b = er.bounds(name, "MANY")
    with torch.no_grad():
        got = er.restated_encode_many(sd, txt, mutant="packed")
        got32 = er.restated_encode_many(sd, txt, dtype=torch.float32, mutant="packed")
    dev, dev32 = er.per_row(got[-1], e64[-1]), er.per_row(got32[-1], e64[-1])
    assert dev > b["bound_row"], (name, dev, b["bound_row"])
    print(f"{name} packed: last text of MANY ({len(txt)} texts, first packed row {(len(txt) - 1) * (er.MANY_TOKENS + 1)}): largest per-row "
          f"deviation {dev:.3e} in fp64, {dev32:.3e} in fp32; bound_row {b['bound_row']:.3e}: "
          f"{'resolved' if dev > b['bound_row'] else 'NOT resolved'}; pooled over all rows {er.pooled(got, e64):.3e}")
    assert er.per_row(got[0], e64[0]) < 1e-12               # the first text sits at packed row 0: untouched
    with torch.no_grad():                                   # the same text first and last: equal rows without the defect, other rows with it
        same = [txt[-1]] + txt[1:]
        clean, bad = er.restated_encode_many(sd, same), er.restated_encode_many(sd, same, mutant="packed")
    assert er.per_row(clean[0], clean[-1]) < 1e-12
    assert not torch.equal(bad[0], bad[-1]) and er.per_row(bad[0], bad[-1]) > 1e-9


# ---------------------------------------------------------------- 3. the packings' kernel forms
@pytest.mark.parametrize("name", ["d512-h8", "d260-h3"])
def test_many_changes_a_gemm_form(name):
    n = er.many_count(name)
    assert n is not None and n == len(er.texts(name, "MANY"))
    M = er.rows_of(er.token_counts(name, "MANY"))
    a, c = er.forms(name, er.rows_of(er.EDGES)), er.forms(name, M)
    print(f"{name}: EDGES M = {er.rows_of(er.EDGES)} {a}; MANY {n} texts, M = {M} {c}")
    assert M <= er.MAX_ROWS and a != c
    assert er.forms(name, M - er.MANY_TOKENS - 1) == a      # (the fewest texts that do it)
    if name == "d512-h8":                                   # the launch rule, restated: 256 tiles of 128 x 128
        N = max(N for N, _ in er.encoder_gemms(name))
        assert -(-M // 128) * -(-N // 128) >= 256 > -(-(M - er.MANY_TOKENS - 1) // 128) * -(-N // 128)


def test_unreachable_cases_are_listed_and_edges_keep_their_m():
    for name in NAMES:
        assert (er.many_count(name) is None) == (name in er.MANY_UNREACHABLE), name
        assert er.rows_of(er.token_counts(name, "EDGES")) == er.rows_of(er.token_counts(name, "EDGES_REVERSED")) == 1011
        a, r = er.texts(name, "EDGES"), er.texts(name, "EDGES_REVERSED")
        assert all(torch.equal(x, y) for x, y in zip(a, r[::-1]))
    for name in er.MANY_UNREACHABLE:
        assert er.forms(name, er.MAX_ROWS) == er.forms(name, er.rows_of(er.EDGES))


@pytest.mark.parametrize("name", NAMES)
def test_texts_are_seeded_and_hold_neither_pad_nor_eos(name):
    eos = er.state_dict(name)["token_emb.text.weight"].shape[0] - 1
    for packing in er.PACKINGS:
        if packing == "MANY" and name in er.MANY_UNREACHABLE:
            continue
        txt = er.texts(name, packing)
        assert [t.shape[1] for t in txt] == list(er.token_counts(name, packing))
        assert all(t.numel() == 0 or (1 <= int(t.min()) and int(t.max()) < eos) for t in txt)
        assert max(t.shape[1] for t in txt) + 2 <= er.MAX_SOURCE
