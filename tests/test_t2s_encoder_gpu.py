"""GPU: the text2semantic encoder as every call runs it - TextToSemanticDecoder.encode_many, several texts packed into one ragged batch -
and the context records _contexts / _guided_contexts scatter its output into (t2s.py), against the fp64 oracle (oracle/t2s_oracle.py),
text by text and row by row.  Cases, packings, expectations, metrics and bounds: tests/t2s_encoder_restated.py; what the bounds resolve:
tests/test_t2s_encoder.py (CPU).  Three models (cosingle_small: width 64, 1 head, depth 2; d260-h3: K % 32 != 0; d512-h8), max_source
272; packings EDGES (rows 2 .. 257 around the 32-key tile and the 128-query block, the eos-only text, 270 tokens), EDGES_REVERSED and
MANY (32-token texts until an encoder GEMM changes its form: 43 texts / 1419 rows for d512-h8, 90 / 2970 for d260-h3; width 64 cannot
get there under 4096 rows and is skipped by name).

  encoder vs fp64    every text of encode_many within bound_text / bound_row = 4x the fp32 CPU oracle's own distance from fp64 over the
                     packing's texts; the Ragged's lengths and cu as expected;
  neighbours         a text's rows bit-equal in EDGES and EDGES_REVERSED (same M, same forms, another offset); encode(text) alone
                     bit-equal to its rows in the packing wherever gemm_f32_form agrees for all four GEMMs, else within the fp64 bounds
                     with the outcome of the bit comparison printed (MANY: the first and the last text); the same call twice bit-equal;
  context records    kv_c of every decoder layer pre-filled with a sentinel, _contexts(EDGES, rows=an unordered list with gaps that
                     names the last record): row 0 == the null row bit for bit, rows 1 .. t within the bounds of enc64 @ W^T in fp64,
                     counts t + 1, everything else still the sentinel; the 270-token text (271 rows with its eos) ends at index
                     max_source - 1 and its count is max_source.  _guided_contexts: record 2u bit-equal to what _contexts wrote, record
                     2u + 1 the null row and nothing else, counts [c, 1, ...];
  behind a count     8 decode steps (generate, collect_logits, fixed draws) plainly, and with every kv_c row at or behind the
                     utterance's count - and every record it does not use - overwritten with NaN between _contexts and the first step:
                     tokens and logits bit-equal and finite; the same under cond_scale 1.5 (rows behind the null row of the odd record).

MEASURED (MI355X) - a record, not a threshold.  Worst per text / per row of the GPU against fp64, and the fp32 CPU oracle's own figures
(on the same host) that the bounds are 4x of:
    case            packing  M     GPU per text  per row    fp32 CPU per text  per row    GEMM forms (to_qkv, to_out, ff.1, ff.4)
    cosingle_small  EDGES    1011  8.527e-07     1.838e-06  8.203e-07          1.969e-06  T64 T64 T64 T64_GENERIC
    d260-h3         EDGES    1011  9.473e-07     1.362e-06  7.405e-07          1.240e-06  T64_GENERIC T64 T64_GENERIC T64_GENERIC
    d260-h3         MANY     2970  9.923e-07     1.427e-06  7.683e-07          1.198e-06  T64_GENERIC T64 T128_GENERIC T64_GENERIC
    d512-h8         EDGES    1011  1.346e-06     1.696e-06  8.338e-07          1.078e-06  T64 T64 T64 T64_GENERIC
    d512-h8         MANY     1419  1.374e-06     1.740e-06  8.261e-07          1.122e-06  T64 T64 T128_DMA T64_GENERIC
(EDGES_REVERSED: the figures of EDGES, bit for bit.)  The closest any text came to a bound: 0.42 of bound_text, 0.39 of bound_row (d512-h8).
Context rows, worst layer:  cosingle_small 8.720e-07 / 2.019e-06 (fp32 CPU product 8.471e-07 / 1.943e-06), d260-h3 1.014e-06 / 1.439e-06
(7.925e-07 / 1.363e-06), d512-h8 1.401e-06 / 1.787e-06 (8.613e-07 / 1.141e-06).
Bit-equality HELD ACROSS THE FORM CHANGES: the first and the last text of MANY encoded alone (all four GEMMs on 64-row tiles) equal
their rows in the packing (ff.1 on T128_GENERIC / T128_DMA) bit for bit, in both cases - every form of the fp32 GEMM walks K in the same
order.  All exact checks (offsets, alone, twice, null rows, sentinels, counts, NaN behind the counts) hold in every case.  No wrong
result was found; no kernel or host code changed.  25 tests (2 skipped by name: cosingle_small x MANY) in 3.4 s.

TRIED, not committed - wrong-value changes to the host code in t2s.py / ops.py (all in bounds), and the tests of this file that failed:
    rotary tables at the packed row index (Ragged.positions)   encoder vs fp64 in all 8 runs (1.02 - 1.4x the bound), offsets 3 / 3,
                                                               alone x EDGES 3 / 3, context records 3 / 3
    the eos row embedded with the neighbouring id              encoder vs fp64 8 / 8 (per text 0.08 - 1.3), alone x MANY 2 / 2, records 3 / 3
    context rows one row late, the null row at index 1         context records 3 / 3, nothing else
    a slot record's key count one too large                    behind a count 4 / 4 (NaN logits), nothing else
"""
import os

import pytest
import torch

import t2s_encoder_restated as er

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = 12345.0
NAMES = list(er.CASES)
RECORDS = (19, 3, 9, 0, 12, 7, 1, 14, 5, 10)        # dialogue records of the ten EDGES texts: unordered, with gaps, the last allocated one first
N_RECORDS = 20
STEPS, MAX_LENGTH = 8, 64
torch.set_num_threads(min(16, os.cpu_count() or 1))

_MODEL, _ENC = {}, {}


def model(name):
    if name not in _MODEL:
        from covomix_amd.t2s import TextToSemanticDecoder
        _MODEL[name] = TextToSemanticDecoder(er.state_dict(name), DEV, max_length=MAX_LENGTH, max_source=er.MAX_SOURCE)
    return _MODEL[name]


def packing_or_skip(name, packing):
    if packing == "MANY" and name in er.MANY_UNREACHABLE:
        pytest.skip(f"{name}: {er.MANY_UNREACHABLE[name]}")


def encoded(name, packing):
    """(rows per text on the host, lengths, cu) of encode_many over a packing: run once, shared, never modified"""
    if (name, packing) not in _ENC:
        enc, rg = model(name).encode_many(er.texts(name, packing))
        _ENC[(name, packing)] = (er.split_rows(enc.cpu(), rg.lengths), list(rg.lengths), rg.cu.cpu().tolist())
    return _ENC[(name, packing)]


def worst(parts, refs):
    """(largest per-text distance, largest per-row distance, (text, row) of the latter)"""
    rows = [er.row_errors(a, r) for a, r in zip(parts, refs)]
    i = max(range(len(rows)), key=lambda j: float(rows[j].max()))
    return max(er.per_text(a, r) for a, r in zip(parts, refs)), float(rows[i].max()), (i, int(rows[i].argmax()))


# ---------------------------------------------------------------- 1. the encoder against fp64
@pytest.mark.parametrize("packing", er.PACKINGS)
@pytest.mark.parametrize("name", NAMES)
def test_encode_many_vs_fp64_oracle(name, packing):
    packing_or_skip(name, packing)
    parts, lengths, cu = encoded(name, packing)
    want = [t + 1 for t in er.token_counts(name, packing)]
    assert lengths == want and cu == [sum(want[:i]) for i in range(len(want) + 1)]
    e64, _ = er.expectation(name, packing)
    b = er.bounds(name, packing)
    assert all(torch.isfinite(p).all() and p.shape == r.shape for p, r in zip(parts, e64))
    text, row, at = worst(parts, e64)
    print(f"{name} {packing} ({len(want)} texts, M = {cu[-1]}, forms {er.forms(name, cu[-1])}): GPU per text {text:.3e}, per row {row:.3e} "
          f"(text {at[0]}, row {at[1]}); fp32 CPU oracle per text {b['ref_text']:.3e}, per row {b['ref_row']:.3e}; "
          f"bounds {b['bound_text']:.3e} / {b['bound_row']:.3e}")
    for i, (p, r) in enumerate(zip(parts, e64)):
        assert er.per_text(p, r) <= b["bound_text"], (name, packing, i, er.per_text(p, r), b["bound_text"])
        assert er.per_row(p, r) <= b["bound_row"], (name, packing, i, er.per_row(p, r), b["bound_row"])


# ---------------------------------------------------------------- 2. independence of neighbours
@pytest.mark.parametrize("name", NAMES)
def test_rows_do_not_depend_on_the_offset(name):
    a, la, _ = encoded(name, "EDGES")
    r, lr, _ = encoded(name, "EDGES_REVERSED")
    assert la == lr[::-1]
    for i, (x, y) in enumerate(zip(a, r[::-1])):
        assert torch.equal(x, y), (name, i, float((x - y).abs().max()))
    again, rg = model(name).encode_many(er.texts(name, "EDGES"))
    assert torch.equal(again.cpu(), torch.cat(a)) and list(rg.lengths) == la


@pytest.mark.parametrize("packing", ["EDGES", "MANY"])
@pytest.mark.parametrize("name", NAMES)
def test_a_text_alone_vs_its_rows_in_the_packing(name, packing):
    packing_or_skip(name, packing)
    parts, lengths, cu = encoded(name, packing)
    txt = er.texts(name, packing)
    e64, _ = er.expectation(name, packing)
    b = er.bounds(name, packing)
    packed_forms = er.forms(name, cu[-1])
    for i in (range(len(txt)) if packing == "EDGES" else (0, len(txt) - 1)):
        alone = model(name).encode(txt[i]).cpu()
        assert alone.shape == parts[i].shape
        same_forms = er.forms(name, lengths[i]) == packed_forms
        equal = torch.equal(alone, parts[i])
        if same_forms:
            assert equal, (name, packing, i, float((alone - parts[i]).abs().max()))
        else:
            print(f"{name} {packing} text {i}: alone {er.forms(name, lengths[i])}, packed {packed_forms}: bit-equal {equal}; alone against fp64 "
                  f"per text {er.per_text(alone, e64[i]):.3e}, per row {er.per_row(alone, e64[i]):.3e}")
            assert er.per_text(alone, e64[i]) <= b["bound_text"] and er.per_row(alone, e64[i]) <= b["bound_row"], (name, packing, i)
    if packing == "MANY":
        assert er.forms(name, lengths[0]) != packed_forms       # (what MANY is for: this branch ran)


# ---------------------------------------------------------------- 3. context records
def fill_records(m):
    m._ensure(8, N_RECORDS, 0)
    assert m._dialogues == N_RECORDS and all(L["kv_c"].shape == (N_RECORDS, er.MAX_SOURCE + 2, 2 * m.d["inner"]) for L in m.dec)
    for L in m.dec:
        L["kv_c"].fill_(SENTINEL)


@pytest.mark.parametrize("name", NAMES)
def test_context_records(name):
    m = model(name)
    txt = er.texts(name, "EDGES")
    e64, _ = er.expectation(name, "EDGES")
    b = er.bounds(name, "EDGES")
    rows = [e.shape[0] for e in e64]
    fill_records(m)
    counts = m._contexts(txt, rows=RECORDS)
    assert counts == [t + 1 for t in rows]
    assert max(RECORDS) == m._dialogues - 1 and len(m.dec) == len(er.kv_weights(name))
    plain = []
    for layer, L in enumerate(m.dec):
        kv, W, null = L["kv_c"].cpu(), L["wkv_c"].cpu(), L["null"].cpu()
        assert torch.equal(W, er.kv_weights(name)[layer])
        res = er.check_records(kv, W, null, RECORDS, e64, SENTINEL)
        print(f"{name} layer {layer}: context rows per text {res['text']:.3e}, per row {res['row']:.3e}; fp32 CPU product per text "
              f"{b['ctx_ref_text']:.3e}, per row {b['ctx_ref_row']:.3e}; bounds {b['ctx_bound_text']:.3e} / {b['ctx_bound_row']:.3e}")
        assert res["null_exact"], (name, layer)
        assert res["untouched"], (name, layer)
        assert res["last"] == rows and res["last"][-1] == er.MAX_SOURCE - 1 and counts[-1] == er.MAX_SOURCE
        for i, (r, e) in enumerate(zip(RECORDS, e64)):
            want = e @ W.double().T
            assert er.per_text(kv[r, 1:rows[i] + 1], want) <= b["ctx_bound_text"], (name, layer, i)
            assert float(res["rows"][i].max()) <= b["ctx_bound_row"], (name, layer, i, float(res["rows"][i].max()))
        plain.append(kv)
    # guided: utterance u in record 2u, the null row alone in record 2u + 1
    fill_records(m)
    counts = m._guided_contexts(txt)
    assert counts == [c for t in rows for c in (t + 1, 1)]
    for layer, L in enumerate(m.dec):
        kv, null = L["kv_c"].cpu(), L["null"].cpu()
        for u, (r, t) in enumerate(zip(RECORDS, rows)):
            assert torch.equal(kv[2 * u, :t + 1], plain[layer][r, :t + 1]), (name, layer, u)
            assert bool((kv[2 * u, t + 1:] == SENTINEL).all()), (name, layer, u)
            assert torch.equal(kv[2 * u + 1, 0], null) and bool((kv[2 * u + 1, 1:] == SENTINEL).all()), (name, layer, u)
        assert bool((kv[2 * len(rows):] == SENTINEL).all())


# ---------------------------------------------------------------- 4. nothing behind a count is read
def decode(m, text, uni, scale, monkeypatch, poison):
    """(streams, logits) of 8 steps; poison: NaN into every kv_c row at or behind its record's count once the contexts are written"""
    name = "_guided_contexts" if scale > 1.0 else "_contexts"
    host, seen = getattr(m, name), []

    def contexts(*a, **k):
        ctx = host(*a, **k)
        for L in m.dec:
            for r in range(L["kv_c"].shape[0]):
                L["kv_c"][r, (ctx[r] if r < len(ctx) else 0):] = float("nan")
        seen.append(list(ctx))
        return ctx
    with monkeypatch.context() as mp:
        if poison:
            mp.setattr(m, name, contexts)
        _, streams, logits = m.generate(text, uniforms=uni, collect_logits=True, cond_scale=scale)
    assert len(seen) == (1 if poison else 0)
    if poison:
        assert seen[0] == ([text.shape[1] + 2, 1] if scale > 1.0 else [text.shape[1] + 2])
        assert all(bool(torch.isnan(L["kv_c"][0, text.shape[1] + 2:]).all()) for L in m.dec)     # (and the decode wrote nothing there)
    return streams.cpu(), logits.cpu()


@pytest.mark.parametrize("scale", [1.0, 1.5], ids=["plain", "guided"])
@pytest.mark.parametrize("name", ["cosingle_small", "d260-h3"])
def test_rows_behind_a_count_are_not_read(name, scale, monkeypatch):
    m = model(name)
    text = er.texts(name, "EDGES")[1]                   # 30 tokens: 32 context rows, one 32-key tile exactly
    uni = torch.rand(STEPS, 1, m.d["vocab"], generator=torch.Generator().manual_seed(5))
    for L in m.dec:
        L["kv_c"].zero_()
    s0, l0 = decode(m, text, uni, scale, monkeypatch, False)
    s1, l1 = decode(m, text, uni, scale, monkeypatch, True)
    print(f"{name} cond_scale {scale}: {l0.shape[0]} steps, tokens {s0.tolist()}")
    assert 1 <= l0.shape[0] <= STEPS and l0.shape[1:] == (1, m.d["vocab"])
    assert torch.isfinite(l0).all() and torch.isfinite(l1).all()
    assert torch.equal(s0, s1) and torch.equal(l0, l1)
    for L in m.dec:
        L["kv_c"].zero_()
