"""GPU: the text2semantic decode (csrc/t2s_decode.hip through t2s.py) at the GEOMETRY edges its ABI admits - target widths 4 .. 4096
that are no multiple of a 256-float strip or exceed one 1024-float chunk, 1 / 2 / 3 heads, vocabularies 5 .. 1024 (odd ones included),
feed-forward widths up to 4096 with 0 / 1 / 3 padded entries, two outputs with an odd slice offset - against the fp64 oracle
(oracle/t2s_oracle.py).  Every other GPU test of the decode runs one of four geometries (widths 64 / 128 / 512 / 1024, vocab 502);
gemv_kernel, attn_kernel and the sampling kernels have no entry point of their own, so the shapes they see are those of the model.

The cases, what each launches and the restated launch arithmetic live in tests/t2s_geometry.py; tests/test_t2s_geometry.py (CPU) holds
the table to it (every path class is reached by a case and by none of the four fixture geometries) and shows that the oracle resolves
a lost 4-vector, output row or logit on exactly these models while its own fp32 restatement stays inside the bound.  Models: depth 1,
source width 64, synthetic weights (seed 0), a 7-token text, 48 steps, max_length 64, max_source 16.  Per case:

  one slot vs fp64   step logits of generate_batch(collect_logits, ignore_eos) against teacher_forced_logits on the GPU's OWN tokens:
                     per-position rel-L2 <= LONG_LOGIT_TOL = 1.5e-5 (the project's bound, not tuned); the token == reference_choice on
                     every decidable step; decidable share >= 0.9 per case, >= 0.98 pooled;
  slot forms         the utterance next to 1, 2, 4 and 8 others of different text length (2, 3, 5, 9 slots: BQ = 2, 4, 8 and two slot
                     groups): every utterance's tokens and logits bit-identical to its run alone;
  padding            with h and the logits pre-filled with NaN / a sentinel: h[:, ff_inner:ff_inner_pad] of the launched slot groups is
                     exactly zero after a step, their logits hold no NaN, and the logits rows of the slots outside the launched groups
                     (the launch computes whole groups of 1 / 2 / 4 / 8 slots) keep the sentinel;
  n_ctx > 0          the host's descriptor with n_ctx = the slot's context row count (AttnArgs.n_fixed >= 0): bit-identical to n_ctx == 0;
                     n_ctx = 1 (the null key alone) is not - the field is honoured;
and once: guidance (k260-h3-v501, cond_scale 2, combined logits against the oracle's two passes) and the refusals (width 4100,
ff_inner_pad 4100, vocab 1025, two outputs at width 1028 / 1032: CVX_EINVAL "bad dimensions", nothing written).

MEASURED (MI355X) - a record, not a threshold.  "kernel": max per-position rel-L2 of the step logits against fp64, one slot; "fp32": the
same figure of the oracle restated in fp32 on the CPU (tests/test_t2s_geometry.py, random forced tokens); decidable share; mismatching
tokens on decidable steps:
    case              kernel      fp32        decidable  mismatches
    k4-v5             8.755e-07   1.978e-06   1.0000     0
    k260-h3-v501      7.445e-07   1.048e-06   1.0000     0
    k1020-h2-v1023    5.610e-07   1.244e-06   1.0000     0
    k1028-h1-v1024    4.262e-07   9.901e-07   1.0000     0
    k1536-ff4096      3.656e-07   8.707e-07   1.0000     0
    k4096-v65         4.830e-07   8.139e-07   1.0000     0
    k64-ff4095        6.368e-07   1.393e-06   0.9792     0
    two-k520-v333     6.547e-07   1.213e-06   0.9896     0
    two-k8-v9         4.429e-07   8.716e-07   1.0000     0
    pooled                                    0.9962 (of 528 steps)
    k260-h3-v501, cond_scale 2: kernel 5.783e-07, decidable 1.0000, 0 mismatches.
Slot forms, padding, n_ctx and the refusals are exact checks: all hold, in every case.  No wrong result at any edge; no kernel or host
code changed.

TRIED, not committed - six wrong-value changes to t2s_decode.hip in one build (all in bounds), and the tests of this file that failed; its
other 16 tests passed:
    the sum of squares not carried into the second chunk     one slot vs fp64: k1028 (rel-L2 17), k1536 (1.3), k4096 (1.5)
    the last logit of an odd vocabulary left at 0            one slot vs fp64: k4 (0.32), k260 (0.081), k1020 (0.038), both two-output cases
    the logits slice offset rounded down to 64               one slot vs fp64: two-k520 (1.1), two-k8 (0.88)
    BQ = 8 staging drops a partial strip behind whole ones under the norm   slot forms from 5 slots on: k260, k1020, k1028, two-k520
    the zero fill of exactly one entry skipped               padding: k64-ff4095 alone, at one slot
    a fixed key count one short                              n_ctx > 0: every case
"""
import ctypes as C
import os

import pytest
import torch

import t2s_geometry as tg
import t2s_oracle as orc

pytestmark = pytest.mark.gpu

TOL = orc.LONG_LOGIT_TOL
EINVAL = -22
SENTINEL = 12345.0
DEV = torch.device("cuda:0")
NAMES = list(tg.CASES)
OTHER_TEXTS = (1, 15, 4, 9, 2, 12, 3, 6)            # token counts of the utterances that share the slots (max_source - 1 = 15)
torch.set_num_threads(min(16, os.cpu_count() or 1))

_MODEL, _ALONE, _TF = {}, {}, {}


def model(name):
    """(state dict, decoder) of a case: built once"""
    if name not in _MODEL:
        from covomix_amd.t2s import TextToSemanticDecoder
        sd = tg.state_dict(name)
        _MODEL[name] = (sd, TextToSemanticDecoder(sd, DEV, max_length=tg.MAX_LENGTH, max_source=tg.MAX_SOURCE))
    return _MODEL[name]


def utterance(name, i):
    """(text, uniform draws) of utterance i of a case: 0 is the 7-token text, the others have OTHER_TEXTS[i - 1] tokens"""
    c = tg.CASES[name]
    src = tg.text() if i == 0 else tg.text(OTHER_TEXTS[i - 1], seed=100 + i)
    return src, tg.draws(tg.STEPS, c["outputs"], c["vocab"], seed=1000 + i)


def alone(name, i=0):
    """(streams [S, L], logits [L, S, V]) of utterance i decoded in one slot, one step at a time: run once, shared, never modified"""
    if (name, i) not in _ALONE:
        c, (_, m) = tg.CASES[name], model(name)
        src, uni = utterance(name, i)
        _, streams, logits = m.generate_batch([src], [uni], collect_logits=True, ignore_eos=True)[0]
        assert streams.shape == (c["outputs"], tg.STEPS) and logits.shape == (tg.STEPS, c["outputs"], c["vocab"])
        _ALONE[(name, i)] = (streams.cpu(), logits.cpu())
    return _ALONE[(name, i)]


def against_fp64(name):
    """(max per-position rel-L2, its position, decidable steps, steps, mismatches on decidable steps) of the one-slot run"""
    if name not in _TF:
        sd, _ = model(name)
        src, uni = utterance(name, 0)
        streams, logits = alone(name)
        with torch.no_grad():
            tf = orc.teacher_forced_logits(sd, src, streams)
        per = orc.per_position_rel_l2(logits.reshape(tf.shape), tf)
        tok, dec = orc.reference_choice(tf, uni)
        _TF[name] = (float(per.max()), int(per.argmax()), int(dec.sum()), dec.numel(), int(((tok.T != streams) & dec.T).sum()))
    return _TF[name]


# ---------------------------------------------------------------- one slot, against fp64
@pytest.mark.parametrize("name", NAMES)
def test_one_slot_vs_fp64_oracle(name):
    e, at, n_dec, n, mism = against_fp64(name)
    print(f"{name}: max per-position logit rel-L2 {e:.3e} (at {at}); decidable {n_dec / n:.4f}; mismatching tokens {mism}")
    assert torch.isfinite(alone(name)[1]).all()
    assert e <= TOL, (name, e)
    assert mism == 0, (name, mism)
    assert n_dec >= 0.9 * n, (name, n_dec, n)


def test_decidable_share_pooled():
    got = [against_fp64(name) for name in NAMES]
    n_dec, n = sum(g[2] for g in got), sum(g[3] for g in got)
    print(f"pooled: decidable {n_dec / n:.4f} of {n} steps")
    assert n_dec >= 0.98 * n, (n_dec, n)


# ---------------------------------------------------------------- slot forms
@pytest.mark.parametrize("name", NAMES)
def test_slot_forms_equal_the_run_alone(name):
    """2, 3, 5 and 9 slots (gemv_kernel<MODE, 2 / 4 / 8>, and two slot groups on the padded grid): the header's promise - the arithmetic
    per utterance does not depend on the batch, the slot or the neighbours - with partial strips under the norm, several chunks, idle
    waves and exiting row blocks."""
    _, m = model(name)
    for slots in tg.SLOT_FORMS[1:]:
        srcs, unis = zip(*(utterance(name, i) for i in range(slots)))
        res = m.generate_batch(list(srcs), list(unis), collect_logits=True, ignore_eos=True)
        for i, (_, streams, logits) in enumerate(res):
            s1, l1 = alone(name, i)
            assert torch.equal(streams.cpu(), s1), (name, slots, i)
            assert torch.equal(logits.cpu(), l1), (name, slots, i, float((logits.cpu() - l1).abs().max()))


# ---------------------------------------------------------------- guidance
def test_guidance_vs_fp64_oracle():
    """cond_scale = 2 on k260-h3-v501 (a slot pair: gemv_kernel<MODE, 2>): the combined logits null + (cond - null) * 2"""
    name = "k260-h3-v501"
    sd, m = model(name)
    src, uni = utterance(name, 0)
    _, streams, logits = m.generate_batch([src], [uni], collect_logits=True, cond_scale=2.0, ignore_eos=True)[0]
    streams, logits = streams.cpu(), logits.cpu()
    assert streams.shape == (1, tg.STEPS)
    with torch.no_grad():
        tf = orc.teacher_forced_logits(sd, src, streams, cond_scale=2.0)
    per = orc.per_position_rel_l2(logits.reshape(tf.shape), tf)
    tok, dec = orc.reference_choice(tf, uni)
    mism = int(((tok.T != streams) & dec.T).sum())
    print(f"{name} cond_scale 2: max per-position logit rel-L2 {float(per.max()):.3e} (at {int(per.argmax())}); "
          f"decidable {float(dec.double().mean()):.4f}; mismatching tokens {mism}")
    assert float(per.max()) <= TOL and mism == 0 and int(dec.sum()) >= 0.9 * dec.numel()


# ---------------------------------------------------------------- padding
@pytest.mark.parametrize("name", NAMES)
def test_padding_is_zeroed_and_other_slots_are_untouched(name):
    _, m = model(name)
    d = m.d
    for slots in (1, 3, 9):
        la = tg.gemv_launches(tg.dims(**tg.CASES[name]), slots)[0]
        group = la["BQ"] * la["groups"]                  # the slots the launches compute: 1, 4 and 16
        assert group == {1: 1, 3: 4, 9: 16}[slots]
        m._ensure(slots, slots, tg.STEPS)
        assert m.buf["h"].shape[0] >= max(8, group) and m.buf["h"].shape[1] == m.Fp == tg.dims(**tg.CASES[name])["ff_inner_pad"]
        m.buf["h"].fill_(float("nan"))
        m.buf["logits"].fill_(SENTINEL)
        srcs, unis = zip(*(utterance(name, i) for i in range(slots)))
        res = m.generate_batch(list(srcs), [u[:2] for u in unis], collect_logits=True, ignore_eos=True)
        h, lg = m.buf["h"].cpu(), m.buf["logits"].cpu()
        assert bool((h[:group, d["ff_tgt"]:] == 0).all()), (name, slots)
        assert torch.isfinite(h[:slots, :d["ff_tgt"]]).all() and torch.isfinite(lg[:slots]).all(), (name, slots)
        assert bool((lg[group:] == SENTINEL).all()), (name, slots)
        assert bool(torch.isnan(h[group:]).all()), (name, slots)
        for i, (_, streams, logits) in enumerate(res):   # NaNs in the padding would have reached the logits through w2
            assert torch.equal(logits.cpu(), alone(name, i)[1][:2]) and torch.equal(streams.cpu(), alone(name, i)[0][:, :2]), (name, slots, i)
        m.buf["h"].zero_()


# ---------------------------------------------------------------- a fixed context count
def run_with_n_ctx(m, n_ctx, src, uni):
    host = m._descriptor

    def descriptor(*a, **k):
        dec = host(*a, **k)
        dec.n_ctx = n_ctx
        return dec
    m._descriptor = descriptor
    try:
        _, streams, logits = m.generate_batch([src], [uni], collect_logits=True, ignore_eos=True)[0]
    finally:
        del m._descriptor
    return streams.cpu(), logits.cpu()


@pytest.mark.parametrize("name", NAMES)
def test_fixed_context_count_equals_the_per_slot_count(name):
    """n_ctx > 0: the cross-attention takes its key count from the descriptor (AttnArgs.n_fixed >= 0), not from the slot record"""
    _, m = model(name)
    src, uni = utterance(name, 0)
    s0, l0 = alone(name)
    rows = tg.TEXT_TOKENS + 2                            # null + text + text eos
    s1, l1 = run_with_n_ctx(m, rows, src, uni)
    assert int(m.buf["state"][0, 3]) == rows             # ... which is what the slot record says
    assert torch.equal(s1, s0) and torch.equal(l1, l0), name
    _, l2 = run_with_n_ctx(m, 1, src, uni[:4])
    assert not torch.equal(l2, l0[:4]), name
    l3 = m.generate_batch([src], [uni[:4]], collect_logits=True, ignore_eos=True)[0][2].cpu()
    assert torch.equal(l3, l0[:4])                       # (the decoder is back on the host's descriptor)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("change", [dict(dim=4100, dim_emb=4100), dict(ff_inner_pad=4100), dict(vocab=1025),
                                    dict(streams=2, dim=1028, dim_emb=514), dict(streams=2, dim=1032, dim_emb=516)],
                         ids=["width-4100", "ff-pad-4100", "vocab-1025", "two-outputs-1028", "two-outputs-1032"])
def test_geometry_past_the_limits_is_refused(change):
    """t2s_validate: CVX_EINVAL "bad dimensions" before anything is launched - the buffers of the descriptor keep their contents"""
    from covomix_amd import _lib, ops
    lib = _lib.load()
    _, m = model("k260-h3-v501")
    alone("k260-h3-v501")                                # (buffers allocated and holding a finished decode)
    dec = m._descriptor(1.0, 1)
    assert lib.cvx_t2s_decode_steps(C.byref(dec), 0, ops._stream()) == 0       # the unchanged descriptor is accepted (0 steps: no launch)
    for k, v in change.items():
        assert hasattr(dec, k)
        setattr(dec, k, v)
    names = ("x", "q", "att", "h", "logits", "tokens", "state")
    torch.cuda.synchronize()
    before = {n: m.buf[n].clone() for n in names}
    rc = lib.cvx_t2s_decode_steps(C.byref(dec), 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == EINVAL, (change, rc)
    assert b"bad dimensions" in lib.cvx_last_error_string()
    for n in names:
        assert torch.equal(m.buf[n], before[n]), (change, n)
