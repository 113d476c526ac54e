"""CPU: the history rules of the text2semantic decode (repetition penalty, no-repeat n-gram, minimum length; include/covomix_hip.h,
cvx_t2s_decode_steps_rules).
  * tests/t2s_rules_restated.py equals a brute-force loop over the definition on random rows, bit for bit;
  * host-side validation (t2s.check_rules), the table layout (t2s.rules_rows), the untouched settings table, the C header, the ctypes
    binding, the command line and the side files;
  * the new kernels of the built library use no scratch;
  * the caps the GPU tests of tests/test_t2s_rules_gpu.py rely on hold on the CPU oracle alone (its `top_k_filter` wrapped): under every
    rule set the decodes are mostly decidable and never fall back, and WITHOUT rules the same decodes repeat 2-grams and, under the default
    filter, cosingle_small ends before step 40 - which is what lets those GPU tests fail."""
import inspect
import json
import math
import os
import re
from unittest import mock

import pytest
import torch

import t2s_filter_restated as fr
import t2s_rules_restated as rr
from test_t2s_filters import DECODE_STEPS, decode_uniforms, load_small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE_SETS = {"penalty": (1.3, 16, 0, 0), "ngram2": (1.0, 0, 2, 0), "ngram3_penalty": (1.3, 0, 3, 0), "min40": (1.0, 0, 0, 40)}
DECODE_KS = (7, 1)
THETAS = (1.0, 1.3, 2.0, 0.5)


def brute_rules(logits, h, rules, eos):
    """the definition, entry by entry, in python; fp32 arithmetic through one-element tensors"""
    theta, W, n, m = rules
    h = [int(x) for x in h]
    pos, V = len(h), logits.numel()
    th = torch.tensor(theta, dtype=torch.float32)
    seen = set(h[max(0, pos - W):pos] if W > 0 else h)
    l = [logits[i].clone() for i in range(V)]
    for i in range(V):
        if i in seen:
            l[i] = l[i] / th if float(l[i]) > 0 else l[i] * th
    banned = set()
    if n >= 1 and pos >= n - 1:
        for j in range(0, pos - n + 1):
            if h[j:j + n - 1] == h[pos - n + 1:pos]:
                banned.add(h[j + n - 1])
    if pos < m:
        l[eos] = torch.tensor(float("-inf"))
    with_bans = [torch.tensor(float("-inf")) if i in banned else l[i] for i in range(V)]
    void = not any(math.isfinite(float(x)) for x in with_bans)
    return torch.stack(l if void else with_bans), void


def random_row(gen, V):
    l = torch.randn(V, generator=gen) * 3
    l[torch.rand(V, generator=gen) < 0.1] = 0.0
    l[torch.rand(V, generator=gen) < 0.1] = -0.0
    l[torch.rand(V, generator=gen) < 0.1] = float("-inf")
    return l


@pytest.mark.parametrize("n", range(9))
def test_restatement_equals_the_brute_force_loop(n):
    gen = torch.Generator().manual_seed(100 + n)
    V, eos, cases = 12, 11, 0
    for length in sorted({0, max(n - 1, 0), n, 1, 2, 7, 8, 30}):
        for W in (0, 1, 7, length + 3):
            for theta in THETAS:
                for m in (0, length + 1):
                    h = torch.randint(0, 4 if length > 8 else V, (length,), generator=gen)      # (few ids: n-grams do repeat)
                    l = random_row(gen, V)
                    got, void = rr.apply_rules(l, h, (theta, W, n, m), eos)
                    want, wvoid = brute_rules(l, h, (theta, W, n, m), eos)
                    assert void == wvoid and torch.equal(got.view(torch.int32), want.view(torch.int32)), (n, length, W, theta, m, h.tolist())
                    cases += 1
    assert cases == len({0, max(n - 1, 0), n, 1, 2, 7, 8, 30}) * 4 * 4 * 2


def test_all_banned_row_falls_back():
    """V = 5 and a history that bans every id: the bans are void, the penalty and the eos suppression stay"""
    l = torch.tensor([1.0, -2.0, 0.5, 3.0, 0.25])
    h = torch.tensor([0, 1, 2, 3, 4])
    got, void = rr.apply_rules(l, h, (2.0, 0, 1, 0), 4)
    assert void and got.tolist() == [0.5, -4.0, 0.25, 1.5, 0.125]
    got, void = rr.apply_rules(l, h, (2.0, 0, 1, 6), 4)
    assert void and got.tolist() == [0.5, -4.0, 0.25, 1.5, float("-inf")]
    want, wvoid = brute_rules(l, h, (2.0, 0, 1, 6), 4)
    assert wvoid and torch.equal(got, want)
    got, void = rr.apply_rules(l, h[:4], (1.0, 0, 1, 0), 4)                 # one id left: no fallback
    assert not void and got.tolist() == [float("-inf")] * 4 + [0.25]
    # 2-grams: (0 1) and (0 2) seen, the history ends in 0 -> 1 and 2 banned
    got, void = rr.apply_rules(l, torch.tensor([0, 1, 0, 2, 0]), (1.0, 0, 2, 0), 4)
    assert not void and got.tolist() == [1.0, float("-inf"), float("-inf"), 3.0, 0.25]


def test_check_rules_and_rows():
    from covomix_amd import _lib
    from covomix_amd.t2s import UtteranceSettings, check_rules, check_settings, rules_active, rules_rows, settings_rows
    assert check_rules(None, 2, 64) == [(1.0, 0, 0, 0)] * 2 and not rules_active(check_rules(None, 2, 64))
    got = check_rules([None, {"repetition_penalty": 2, "min_length": 7}, UtteranceSettings(no_repeat_ngram_size=8, repetition_window=5),
                       {"temperature": 0.5}], 4, 64, 1.3, 16, 2, 3)
    assert got == [(1.3, 16, 2, 3), (2.0, 16, 2, 7), (1.3, 5, 8, 3), (1.3, 16, 2, 3)] and rules_active(got)
    assert not rules_active([(1.0, 9, 0, 0)]) and rules_active([(1.0, 0, 0, 1)]) and rules_active([(0.5, 0, 0, 0)])
    rows = rules_rows(got)
    assert rows.dtype == torch.int32 and rows.shape == (4, _lib.T2S_RULES_WORDS) == (4, 4)
    assert rows[:, 0].view(torch.float32).tolist() == [torch.tensor(x, dtype=torch.float32).item() for x in (1.3, 2.0, 1.3, 1.3)]
    assert rows[:, 1:].tolist() == [[16, 2, 3], [16, 2, 7], [5, 8, 3], [16, 2, 3]]
    assert rules_rows([]).shape == (0, 4)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
               dict(repetition_penalty=float("inf")), dict(repetition_penalty="x"), dict(repetition_window=-1), dict(repetition_window=1.5),
               dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=True), dict(min_length=-1),
               dict(min_length=65)):
        with pytest.raises(ValueError):
            check_rules(None, 1, 64, **kw)
        with pytest.raises(ValueError):
            check_rules([kw], 1, 64)
    assert check_rules(None, 1, 64, min_length=64, no_repeat_ngram_size=8) == [(1.0, 0, 8, 64)]
    with pytest.raises(ValueError):
        check_rules([None], 2, 64)
    # the settings table is untouched: same tuples, same 8-word rows, words 6 and 7 zero - whatever rule fields an entry carries
    res = check_settings([{"temperature": 0.5, "min_length": 3, "repetition_penalty": 1.3}, None], 2, 502)
    assert res == check_settings([{"temperature": 0.5}, None], 2, 502) == [(0.5, (0, 51, 0.0), 1.0), (1.0, (0, 51, 0.0), 1.0)]
    srows = settings_rows(res, [3, 0])
    assert srows.shape == (2, 8) and srows[:, 6:].tolist() == [[0, 0], [0, 0]] and srows[:, 5].tolist() == [3, 0]
    with pytest.raises(ValueError):
        check_settings([{"repetition": 1.3}], 1, 502)


def test_header_binding_and_version():
    import ctypes as C
    from covomix_amd import _lib
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "covomix_hip.h")).read())
    assert "#define CVX_ABI_VERSION 113" in hdr and _lib.ABI_VERSION == 113
    assert ("int cvx_t2s_decode_steps_rules(const cvx_t2s_decoder* dec, const cvx_t2s_scoring* scoring, const cvx_t2s_per_dialogue* per, "
            "const cvx_t2s_mixed* mixed, const cvx_t2s_rules* rules, int32_t n_steps, cvx_stream_t stream);") in hdr
    assert ("int cvx_t2s_rules_f32(const float* logits, const int64_t* history, const int32_t* hist_len, const void* table, int64_t rows, "
            "int32_t V, int32_t hist_ld, int32_t eos_id, float* out, cvx_stream_t stream);") in hdr
    assert "typedef struct cvx_t2s_rules { uint32_t struct_size; int32_t n_records; const void* table; } cvx_t2s_rules;" in hdr
    assert "typedef struct cvx_t2s_per_dialogue { uint32_t struct_size; int32_t n_records; const void* table; } cvx_t2s_per_dialogue;" in hdr
    assert _lib.T2SRules._fields_ == [("struct_size", C.c_uint32), ("n_records", C.c_int32), ("table", C.c_void_p)]
    assert _lib.T2SPerDialogue._fields_ == _lib.T2SRules._fields_ and C.sizeof(_lib.T2SRules) == 16
    assert _lib.T2S_PER_WORDS == 8 and _lib.T2S_RULES_WORDS == 4
    res, args = _lib.SIGNATURES["cvx_t2s_decode_steps_rules"]
    assert res is C.c_int and args == [C.POINTER(_lib.T2SDecoder), C.POINTER(_lib.T2SScoring), C.POINTER(_lib.T2SPerDialogue),
                                       C.POINTER(_lib.T2SMixed), C.POINTER(_lib.T2SRules), C.c_int32, C.c_void_p]
    res, args = _lib.SIGNATURES["cvx_t2s_rules_f32"]
    assert res is C.c_int and args == [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib = _lib.load()
    assert lib.cvx_version() == 113 and lib.cvx_t2s_decode_steps_rules and lib.cvx_t2s_rules_f32


def test_cli_flags_and_side_files_reach_the_facade(tmp_path):
    from covomix_amd import generation
    from covomix_amd.conditional_model import CoVoMixModel
    from covomix_amd.t2s import RULE_FIELDS, TextToSemanticDecoder, UtteranceSettings
    p = generation.build_parser()
    assert generation.t2s_sampling_kwargs(p.parse_args([])) == {}
    a = p.parse_args(["--t2s_repetition_penalty", "1.3", "--t2s_repetition_window", "16", "--t2s_no_repeat_ngram", "3", "--t2s_min_length", "40"])
    kw = generation.t2s_sampling_kwargs(a)
    assert kw == dict(repetition_penalty=1.3, repetition_window=16, no_repeat_ngram_size=3, min_length=40)
    assert set(kw) == set(RULE_FIELDS) <= set(UtteranceSettings._fields)
    for fn in (CoVoMixModel.synthesis_sample_text2semantic, TextToSemanticDecoder.generate, TextToSemanticDecoder.generate_batch,
               TextToSemanticDecoder.generate_many, TextToSemanticDecoder.generate_beam, TextToSemanticDecoder.generate_beam_many):
        params = inspect.signature(fn).parameters
        assert [params[f].default for f in RULE_FIELDS] == [1.0, 0, 0, 0], fn
    with pytest.raises(ValueError):
        generation.t2s_sampling_kwargs(p.parse_args(["--t2s_beam_size", "4", "--t2s_no_repeat_ngram", "2"]))
    # the side file of a turn: the same keys as the flags, overriding them
    assert set(generation.T2S_SIDE_FIELDS) >= {"repetition_penalty", "repetition_window", "no_repeat_ngram", "min_length"}
    ids = tmp_path / "utt.text_ids.npy"
    (tmp_path / "utt.t2s.json").write_text(json.dumps({"no_repeat_ngram": 2, "min_length": 5, "temperature": 0.7}))
    side, prefix = generation._turn_side_files(str(tmp_path), "utt", 0, ("ids", str(ids)))
    assert prefix is None and side == {"no_repeat_ngram": 2, "min_length": 5, "temperature": 0.7}
    turn = generation._turn_sampling(kw, side)
    assert turn == dict(temprature=0.7, repetition_penalty=1.3, repetition_window=16, no_repeat_ngram_size=2, min_length=5, filter_fn_kwargs=None)
    assert generation._turn_sampling({}, None) == dict(filter_fn_kwargs=None)
    (tmp_path / "utt.t2s.json").write_text(json.dumps({"no_repeat": 2}))
    with pytest.raises(ValueError):
        generation._turn_side_files(str(tmp_path), "utt", 0, ("ids", str(ids)))


def test_new_kernels_use_no_scratch():
    from covomix_amd import _lib
    from test_attention_form_d import _gfx950_kernel_descriptors
    sym = re.compile(r"_ZN12_GLOBAL__N_1\d+(sample_rules_kernel|sample_mixed_rules_kernel|rules_rows_kernel)([EI].*)")
    found = {}
    for name, (group, private, vgprs) in _gfx950_kernel_descriptors(_lib.LIB_PATH).items():
        m = sym.fullmatch(name)
        if m:
            print(f"FIGURE {name[:70]}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
            found.setdefault(m.group(1), []).append(private)
    assert {k: len(v) for k, v in found.items()} == {"sample_rules_kernel": 2, "sample_mixed_rules_kernel": 2, "rules_rows_kernel": 1}, found
    assert all(p == 0 for v in found.values() for p in v), found


# ---------------------------------------------------------------- the caps of the GPU tests, on the CPU oracle alone
_ORACLE = {}


def oracle_decode(name, k, rules):
    """The CPU oracle's decode of a small fixture, DECODE_STEPS steps with decode_uniforms, top-k = k, under a rule set (None: without):
    its `top_k_filter` is wrapped - the wrapper applies the rules with a history it keeps from its OWN choice (the draws of the step it
    counts), then the restated filter.  -> (logits [L, S, V] before the rules, streams [L, S]); computed once per case."""
    key = (name, k, rules)
    if key not in _ORACLE:
        import t2s_oracle as orc
        g, sd = load_small(name)
        S, V = g["uniforms"].shape[1], g["uniforms"].shape[-1]
        uni = decode_uniforms(S, V)
        hist, calls = [[] for _ in range(S)], [0]

        def wrapped(logits, thres_=None):
            t, s = divmod(calls[0], S)
            calls[0] += 1
            row = logits[0]
            if rules is not None:
                row, _ = rr.apply_rules(row, torch.tensor(hist[s], dtype=torch.int64), rules, V - 1)
            f = fr.filtered(row[None].to(logits.dtype), fr.TOP_K, k)
            hist[s].append(int((f + orc.gumbel_from_uniform(uni[t, s][None])).argmax(dim=-1)))      # (the oracle's own expression at temperature 1)
            return f
        with mock.patch.object(orc, "top_k_filter", wrapped):
            o = orc.generate(sd, torch.from_numpy(g["source_ids"]), uni[:, :, None, :], max_length=DECODE_STEPS)
        streams = o["streams"][0].T
        assert torch.tensor(hist).T.tolist() == streams.tolist()
        _ORACLE[key] = (o["logits"][:, :, 0, :].to(torch.float32), streams, uni)
    return _ORACLE[key]


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
@pytest.mark.parametrize("k", DECODE_KS)
@pytest.mark.parametrize("rules", list(RULE_SETS))
def test_ruled_decode_is_mostly_decidable_on_the_oracle(name, k, rules):
    logits, streams, uni = oracle_decode(name, k, RULE_SETS[rules])
    L, S, V = logits.shape
    tokens, decidable, fallbacks = rr.restated_decode_choice(logits, uni, (1.0, fr.TOP_K, k, 0.0), RULE_SETS[rules], tokens=streams)
    theta, W, n, m = RULE_SETS[rules]
    print(name, k, rules, "steps", L, "undecidable", int((~decidable).sum()), "fallbacks", fallbacks)
    assert torch.equal(tokens[decidable], streams[decidable])
    assert int((~decidable).sum()) <= 0.05 * decidable.numel() and fallbacks == 0
    for s in range(S):
        if n:
            assert rr.repeated_ngrams(streams[:, s], n) == 0
        if m:
            assert L >= min(m, DECODE_STEPS) and not bool((streams[:m, s] == V - 1).any())


@pytest.mark.parametrize("name", ["cosingle_small", "comix_small"])
@pytest.mark.parametrize("k", DECODE_KS)
def test_without_rules_the_decodes_repeat(name, k):
    """what makes the GPU tests able to fail: the rule-free decodes of the same fixtures and draws repeat 2-grams in every stream"""
    _, streams, _ = oracle_decode(name, k, None)
    for s in range(streams.shape[1]):
        rep = rr.repeated_ngrams(streams[:, s], 2)
        print(name, k, "stream", s, "steps", streams.shape[0], "repeated 2-grams", rep)
        assert rep > 0


def test_without_rules_the_default_filter_ends_cosingle_small_early():
    """... and under the default filter (k = 51) cosingle_small samples its eos before step 40: min_length = 40 changes that decode"""
    _, streams, _ = oracle_decode("cosingle_small", 51, None)
    print("cosingle_small default filter: steps", streams.shape[0])
    assert streams.shape[0] < 40 and int(streams[-1, 0]) == 501
