"""GPU: the text2semantic decode (csrc/t2s_decode.hip through t2s.py) at the lengths it is used at - 2048 steps (the CLIs' max_length),
texts up to max_source - 1 tokens, the kernel limits (4096 keys) - against the fp64 oracle (oracle/t2s_oracle.py), not only
against itself.  The oracle is teacher-forced on the GPU's OWN sampled tokens (teacher_forced_logits), so it never drifts from the
decode and every position is a check:
  * logits: at EVERY position, rel-L2 of the GPU's pre-filter step logits against the fp64 pass <= LONG_LOGIT_TOL = 1.5e-5 (a
    maximum over positions: an error in one late 64-key block is not diluted).  Measured on an MI355X: at most 1.4e-6 in every
    case below (the fp32 CPU oracle sits 0.9-1.4e-6 from the fp64 one); with the q projections x8 (case b) 4.7e-5, bounded by
    PEAKED_TOL = 1e-4 - there the fp32 CPU oracle itself is 1.1e-4 (cosingle_small) / 4.0e-4 (comix_small) from fp64: large scores
    through the softmax amplify any fp32 rounding, the decode's included;
  * tokens: the GPU's token == reference_choice (top-k + Gumbel argmax in fp64 from the same uniform draws) on every decidable
    step, and >= 99 % of the steps decidable.
Every run uses ignore_eos (it reaches its full length) and uniforms from a seeded generator.  The oracle's resolving power is
checked on the CPU (tests/test_t2s_oracle_golden.py: one lost key at position 1000, or the lost last context row, exceed the
tolerance at every later position)."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import t2s_oracle as orc

pytestmark = pytest.mark.gpu

KW = {
    "cosingle": dict(two_output=False, dim=512, dim_target=512),
    "comix": dict(two_output=True, dim=512, dim_target=1024),
}
TOL = orc.LONG_LOGIT_TOL
PEAKED_TOL = 1e-4
DEV = torch.device("cuda:0")
torch.set_num_threads(min(16, os.cpu_count() or 1))


def load_sd(name):
    import covomix_amd.synthetic as syn
    g = np.load(os.path.join(GOLDEN, f"t2s_{name}.npz"))
    if name.endswith("_small"):
        return g, {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w::")}
    return g, {k: torch.from_numpy(v) for k, v in syn.t2s_state_dict(syn.t2s_param_shapes(**KW[name]), seed=0).items()}


def peaked(sd, f=8.0):
    """q projections (self- and cross-attention) of the decoder scaled: peaked softmaxes, large scores through the max subtraction"""
    return {k: v * f if k.startswith("target_transformer.") and ".to_q." in k else v for k, v in sd.items()}


_DEC = {}


def decoder(name, max_length=2048, max_source=1024, q_scale=1.0):
    from covomix_amd.t2s import TextToSemanticDecoder
    key = (name, max_length, max_source, q_scale)
    if key not in _DEC:
        g, sd = load_sd(name)
        sd = peaked(sd, q_scale) if q_scale != 1.0 else sd
        _DEC[key] = (g, sd, TextToSemanticDecoder(sd, DEV, max_length=max_length, max_source=max_source))
    return _DEC[key]


def draws(steps, S, V, seed):
    return torch.rand(steps, S, V, generator=torch.Generator().manual_seed(seed))


def text(n, seed, vocab=200):
    """n text ids in 1 .. vocab - 1 (0 is the pad id, the last row of the text embedding the text eos)"""
    return torch.randint(1, vocab, (1, n), generator=torch.Generator().manual_seed(seed))


def check(label, sd, src, uni, streams, logits=None, cond_scale=1.0, temperature=1.0, tol=TOL):
    """the GPU's tokens (streams [S, L]) and optional step logits [L, S, V] against the fp64 teacher-forced pass on those tokens.
    Returns (max per-position rel-L2 or None, decidable steps, total steps, mismatches on decidable steps)."""
    streams = streams.cpu()
    tf = orc.teacher_forced_logits(sd, src, streams, cond_scale=cond_scale)
    L = streams.shape[-1]
    e = None
    if logits is not None:
        per = orc.per_position_rel_l2(logits.reshape(tf.shape), tf)
        e = float(per.max())
    tok, dec = orc.reference_choice(tf, uni[:L].reshape(L, -1, tf.shape[-1]), temperature)
    mism = int(((tok.T != streams) & dec.T).sum())
    n_dec, n = int(dec.sum()), dec.numel()
    print(f"{label}: L={L} max per-position logit rel-L2 {e if e is None else f'{e:.3e}'} (at {None if e is None else int(per.argmax())}); "
          f"decidable {n_dec / n:.4f}; mismatching tokens {mism}")
    assert mism == 0, (label, mism)
    assert e is None or e <= tol, (label, e)
    return e, n_dec, n, mism


def assert_decidable(label, n_dec, n):
    assert n_dec >= 0.99 * n, (label, n_dec, n)


_SINGLE = {}


def single_run(name, steps=2048, q_scale=1.0):
    """one slot, one step at a time with logits: (src, uniforms, streams [S, L], logits [L, S, V])"""
    key = (name, steps, q_scale)
    if key not in _SINGLE:
        g, sd, model = decoder(name, q_scale=q_scale)
        S, V = model.d["streams"], model.d["vocab"]
        src = torch.from_numpy(g["source_ids"])
        uni = draws(steps, S, V, seed=1000 + len(name))
        flat, streams, logits = model.generate_batch([src], [uni], collect_logits=True, ignore_eos=True)[0]
        assert streams.shape == (S, steps) and logits.shape == (steps, S, V)
        _SINGLE[key] = (src, uni, streams.cpu(), logits.cpu())
    return _SINGLE[key]


# ---------------------------------------------------------------- a. full length, one slot
@pytest.mark.slow
@pytest.mark.parametrize("name", ["cosingle_small", "comix_small", "cosingle", "comix"])
def test_full_length_single_slot_vs_fp64_oracle(name):
    _, sd, _ = decoder(name)
    src, uni, streams, logits = single_run(name)
    e, n_dec, n, _ = check(f"a {name}", sd, src, uni, streams, logits)
    assert_decidable(name, n_dec, n)


# ---------------------------------------------------------------- b. peaked attention
@pytest.mark.slow
@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_peaked_attention_vs_fp64_oracle(name):
    """q projections x8: single keys decide the attention output (synthetic weights give diffuse softmaxes otherwise).  The logit
    bound is PEAKED_TOL (module docstring: fp32 arithmetic alone moves these logits by up to 4e-4); a lost key moves them by O(1)."""
    _, sd, _ = decoder(name, q_scale=8.0)
    src, uni, streams, logits = single_run(name, q_scale=8.0)
    stats = []
    orc.teacher_forced_logits(sd, src, streams[:, :512], stats=stats)
    peak = sum(stats) / len(stats)
    print(f"b {name}: mean largest softmax probability of the attention rows {peak:.3f} (unscaled weights: about 0.12)")
    assert peak > 0.5
    e, n_dec, n, _ = check(f"b {name} q x8", sd, src, uni, streams, logits, tol=PEAKED_TOL)
    assert_decidable(name, n_dec, n)


# ---------------------------------------------------------------- c. long texts
@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_long_texts_vs_fp64_oracle(name):
    """cross-attention over 3 .. 1025 context keys (null + text + text eos), across 64-key block boundaries; one lock-step batch."""
    _, sd, model = decoder(name)
    S, V = model.d["streams"], model.d["vocab"]
    lengths = [1, 63, 64, 65, 577, 1023]
    srcs = [text(n, seed=n) for n in lengths]
    unis = [draws(300, S, V, seed=50 + n) for n in lengths]
    res = model.generate_batch(srcs, unis, collect_logits=True, ignore_eos=True)
    tot_dec = tot = 0
    for n_txt, src, uni, (_, streams, logits) in zip(lengths, srcs, unis, res):
        _, n_dec, n, _ = check(f"c {name} text {n_txt}", sd, src, uni, streams, logits)
        tot_dec, tot = tot_dec + n_dec, tot + n
    assert_decidable(name, tot_dec, tot)


# ---------------------------------------------------------------- d. at the kernel limits
@pytest.mark.slow
def test_kernel_limits_4096_steps_and_4096_context_rows():
    """max_length = 4096 = T2S_MAX_KEYS (the LDS score buffer) decoded to the end; max_source = 4094 (ctx_rows = 4096) with a
    4093-token text (4095 context keys)."""
    g, sd, model = decoder("cosingle_small", max_length=4096, max_source=4094)
    S, V = model.d["streams"], model.d["vocab"]
    src = torch.from_numpy(g["source_ids"])
    uni = draws(4096, S, V, seed=4096)
    _, streams, logits = model.generate_batch([src], [uni], collect_logits=True, ignore_eos=True)[0]
    assert streams.shape == (S, 4096)
    _, n_dec, n, _ = check("d max_length 4096", sd, src, uni, streams, logits)
    assert_decidable("4096 steps", n_dec, n)
    src = text(4093, seed=4093)
    uni = draws(300, S, V, seed=4094)
    _, streams, logits = model.generate_batch([src], [uni], collect_logits=True, ignore_eos=True)[0]
    _, n_dec, n, _ = check("d text of 4093 tokens", sd, src, uni, streams, logits)
    assert_decidable("4093-token text", n_dec, n)
    with pytest.raises(ValueError):                                # the text limit is max_source - 1 tokens (+ the text eos)
        model.generate_batch([text(4094, seed=1)], [uni], max_length=4)


def test_decoder_longer_than_the_kernel_limit_is_refused():
    """max_length = 4097 exceeds the LDS score buffer: refused by the host-side validation (cvx_t2s_decode_steps, before any launch)."""
    from covomix_amd import _lib
    from covomix_amd.t2s import TextToSemanticDecoder
    g, sd = load_sd("cosingle_small")
    model = TextToSemanticDecoder(sd, DEV, max_length=4097)
    with pytest.raises(_lib.CovomixHipError, match="bad dimensions"):
        model.generate(torch.from_numpy(g["source_ids"]), max_length=20)
    with pytest.raises(_lib.CovomixHipError, match="bad dimensions"):
        model.generate(torch.from_numpy(g["source_ids"]), max_length=20, collect_logits=True)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- e. graph and queue paths at length
@pytest.mark.slow
@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
def test_lock_step_graph_batch_at_2048_steps_vs_fp64_oracle(name):
    """8 texts of different length, 2048 steps graph-replayed in lock step: slot 0 (case a's text and draws) bit-identical to the
    single-slot step-by-step run, every slot's tokens against reference_choice."""
    _, sd, model = decoder(name)
    S, V = model.d["streams"], model.d["vocab"]
    src0, uni0, streams0, _ = single_run(name)
    srcs = [src0] + [text(n, seed=70 + n) for n in (1, 5, 30, 64, 65, 200, 700)]
    unis = [uni0] + [draws(2048, S, V, seed=80 + i) for i in range(1, 8)]
    res = model.generate_batch(srcs, unis, ignore_eos=True)
    assert torch.equal(res[0][1].cpu(), streams0)
    tot_dec = tot = 0
    for i, (src, uni, (_, streams)) in enumerate(zip(srcs, unis, res)):
        assert streams.shape == (S, 2048)
        _, n_dec, n, _ = check(f"e {name} lock-step slot {i}", sd, src, uni, streams)
        tot_dec, tot = tot_dec + n_dec, tot + n
    assert_decidable(name, tot_dec, tot)


@pytest.mark.slow
def test_continuous_batching_at_length_vs_fp64_oracle():
    """generate_many: 80 dialogues through 64 slots, step limits over 1 .. 2048 - refills land at late positions and the slots of
    one step sit at very different positions.  EVERY dialogue's tokens against reference_choice; a handful against a single-slot run."""
    _, sd, model = decoder("comix_small")
    S, V = model.d["streams"], model.d["vocab"]
    n = 80
    gen = torch.Generator().manual_seed(3)
    limits = [1, 2, 15, 16, 17, 63, 64, 65, 2047, 2048] + torch.randint(1, 2049, (n - 10,), generator=gen).tolist()
    srcs = [text(int(torch.randint(1, 300, (1,), generator=gen)), seed=200 + j) for j in range(n)]
    base = torch.rand(n, 2048, S, V, generator=gen)
    res = model.generate_many(srcs, [base[j] for j in range(n)], slots=64, limits=limits, ignore_eos=True)
    rec = model.last_records
    assert all(rec[j][3] == 3 and rec[j][4] == limits[j] for j in range(n))
    assert len({rec[j][5] for j in range(n)}) == 64
    tot_dec = tot = 0
    for j in range(n):
        assert res[j][1].shape == (S, limits[j])
        _, n_dec, nn, _ = check(f"e generate_many dialogue {j} (limit {limits[j]}, slot {rec[j][5]})", sd, srcs[j], base[j], res[j][1])
        tot_dec, tot = tot_dec + n_dec, tot + nn
    print(f"e generate_many: {tot} steps, decidable {tot_dec / tot:.4f}")
    assert_decidable("generate_many", tot_dec, tot)
    for j in (0, 8, 9, 40, n - 1):
        alone = model.generate_batch([srcs[j]], [base[j][: limits[j]]], ignore_eos=True)[0]
        assert torch.equal(res[j][1], alone[1].cpu()), j


# ---------------------------------------------------------------- f. guidance and temperature
@pytest.mark.slow
@pytest.mark.parametrize("name", ["cosingle_small", "cosingle"])
def test_guidance_at_1024_steps_vs_fp64_oracle(name):
    """cond_scale = 1.5: the combined logits null + (cond - null) * 1.5 against the oracle's two passes."""
    g, sd, model = decoder(name)
    V = model.d["vocab"]
    src = torch.from_numpy(g["source_ids"])
    uni = draws(1024, 1, V, seed=15)
    _, streams, logits = model.generate_batch([src], [uni], collect_logits=True, cond_scale=1.5, ignore_eos=True)[0]
    assert streams.shape == (1, 1024)
    _, n_dec, n, _ = check(f"f {name} cond_scale 1.5", sd, src, uni, streams, logits, cond_scale=1.5)
    assert_decidable(name, n_dec, n)


@pytest.mark.parametrize("temperature", [0.5, 1.7])
def test_temperature_tokens_vs_fp64_oracle(temperature):
    """the kernel multiplies by 1 / T where the reference divides by T: the tokens on decidable steps must not notice."""
    g, sd, model = decoder("comix_small")
    S, V = model.d["streams"], model.d["vocab"]
    src = torch.from_numpy(g["source_ids"])
    uni = draws(1024, S, V, seed=int(temperature * 10))
    _, streams = model.generate_batch([src], [uni], temperature=temperature, ignore_eos=True)[0]
    _, n_dec, n, _ = check(f"f temperature {temperature}", sd, src, uni, streams, temperature=temperature)
    assert_decidable(f"T {temperature}", n_dec, n)


# ---------------------------------------------------------------- uniform draws cover every position a chunked decode reaches
@pytest.mark.parametrize("nb", [8, 64])
def test_uniform_buffer_covers_whole_chunks(nb):
    """A lock-step decode runs whole chunks of CHUNK steps, and its sampling kernel reads the uniform draws of every position it reaches:
    with max_length not a multiple of CHUNK and nb = the dialogue capacity, the last dialogue row used to read up to CHUNK - 1 steps
    of draws past the end of the buffer.  The buffer holds whole chunks; the tokens are those of a run at the rounded length."""
    from covomix_amd.t2s import CHUNK, TextToSemanticDecoder
    g, sd = load_sd("cosingle_small")
    model = TextToSemanticDecoder(sd, DEV, max_length=2048)
    S, V = model.d["streams"], model.d["vocab"]
    srcs = [text(3 + i % 29, seed=300 + i) for i in range(nb)]
    for m in (1, 15, 17, 20, 33, 2047):
        R = math.ceil(m / CHUNK) * CHUNK
        unis = [draws(R, S, V, seed=400 + i) for i in range(nb)]
        res = model.generate_batch(srcs, [u[:m] for u in unis], ignore_eos=True)
        steps = model._descriptor(1.0, nb).uniform_steps
        assert model._dialogues == nb and steps >= R, (m, steps)
        assert model.buf["uniforms"].numel() >= model._dialogues * steps * S * V
        rounded = model.generate_batch(srcs, unis, ignore_eos=True)
        for i in range(nb):
            assert res[i][1].shape == (S, m)
            assert torch.equal(res[i][1], rounded[i][1][:, :m]), (m, i)
