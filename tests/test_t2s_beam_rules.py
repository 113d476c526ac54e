"""CPU: beam search under the history rules no-repeat n-gram and minimum length (include/covomix_hip.h, cvx_t2s_beam_rules_steps).
  1. tests/t2s_beam_rules_restated.py on the crafted blocks of tests/t2s_beam_restated.py: a neutral row is `select`; no selected token is
     banned; with every id of a stream banned the n-gram bans are void and the eos ban is not; with fewer candidates than B the slots
     beyond them are dead;
  2. / 3. the fp64 oracle search under the rules, and the CONDITIONS the GPU comparison of tests/test_t2s_beam_rules_gpu.py relies on,
     checked with the oracle alone: per case a decidable prefix of at least 12 steps that holds a step whose selection the rules changed
     and a re-parenting;
  4. host validation (t2s.check_beam_rules), the table rows, the parser, the header, the binding, the exported symbols, no scratch."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import t2s_beam_restated as br
import t2s_beam_rules_restated as rr
from t2s_rules_restated import banned_ids
from test_t2s_filters import load_small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(G, n, m):
    t = torch.zeros(G, 4, dtype=torch.int32)
    t[:, 0] = torch.tensor(1.0).view(torch.int32)
    t[:, 2], t[:, 3] = n, m
    return t


# ---------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("V", br.VOCABS)
@pytest.mark.parametrize("S", (1, 2))
def test_restatement_on_the_crafted_blocks(V, S):
    for B in br.BEAMS:
        lg, sc, fin = br.block(B, S, V)
        rows = 3 * B
        for dtype in (torch.float64, torch.float32):
            plain = br.select(lg, sc, fin, B, dtype)
            # a neutral row: the selection without rules, whatever the history
            h = rr.history_block(B, S, V, 12, 2)
            got = rr.select(lg, sc, fin, B, h, torch.full((rows,), 12, dtype=torch.int32), _table(3, 0, 0), dtype)
            assert all(torch.equal(got[k], plain[k]) for k in plain), (B, dtype)
            # n = 2, 12 tokens: no selected token is banned, nothing banned is an eos below m, scores are sums of the model's lp
            for n, m in ((2, 0), (1, 13), (3, 12)):
                h = rr.history_block(B, S, V, 12, n)
                hl = torch.full((rows,), 12, dtype=torch.int32)
                got = rr.select(lg, sc, fin, B, h, hl, _table(3, n, m), dtype)
                lp = br._lp(lg, dtype)
                for r in range(rows):
                    g0 = (r // B) * B
                    if int(got["tokens"][r, 0]) < 0:
                        continue
                    p = g0 + int(got["parents"][r])
                    for s in range(S):
                        tok = int(got["tokens"][r, s])
                        row, void = rr.ban_row(lp[p, s], h[p, s, :12].long(), n, m)
                        assert float(row[tok]) > -math.inf, (B, n, m, r)
                        assert void or tok not in banned_ids(h[p, s, :12].long(), n).tolist()
                        assert not (tok == V - 1 and 12 < m)
                        assert float(got["token_lp"][r, s]) == float(lp[p, s, tok])
    print(f"V = {V}, S = {S}: checked")


@pytest.mark.parametrize("V,n", [(3, 1), (3, 2), (5, 2), (5, 8), (502, 1)])
@pytest.mark.parametrize("S", (1, 2))
def test_void_bans_and_dead_slots(V, n, S):
    """histories that ban every id of [0, V - 1).  With the eos banned too (m = pos + 1) the n-gram bans are void and the eos stays banned;
    with the eos free (m = 0) it is every live hypothesis' only candidate: the step-0 group (one live hypothesis) fills one slot, B - 1 die."""
    pos = rr.cover_len(V, n)
    for B in (1, 2, 3, 10):
        lg, sc, fin = br.block(B, S, V)
        rows = 3 * B
        h = rr.history_block(B, S, V, pos, n, kind="cover")
        hl = torch.full((rows,), pos, dtype=torch.int32)
        assert all(len(banned_ids(h[r, s, :pos].long(), n)) == V - 1 for r in range(rows) for s in range(S))
        void = rr.select(lg, sc, fin, B, h, hl, _table(3, n, pos + 1))
        live = int(((sc > -math.inf) & (fin == 0)).sum())
        assert void["voids"] == live * S
        new = void["tokens"][:, 0] >= 0
        assert bool(new.any()) and not bool((void["tokens"][new] == V - 1).any())         # candidates again, and never the eos
        unruled_but_eos = rr.select(lg, sc, fin, B, h, hl, _table(3, 0, pos + 1))
        assert all(torch.equal(void[k], unruled_but_eos[k]) for k in ("parents", "tokens", "scores", "finished"))
        dead = rr.select(lg, sc, fin, B, h, hl, _table(3, n, 0))
        assert dead["voids"] == 0
        step0 = slice(B, 2 * B)                                                            # (the block's second group: hypothesis 0 alone live)
        assert dead["tokens"][step0][0].tolist() == [V - 1] * S and int(dead["finished"][step0][0]) == 1
        assert dead["scores"][step0][1:].tolist() == [-math.inf] * (B - 1)
        assert dead["parents"][step0].tolist() == [0] + list(range(1, B)) and bool((dead["tokens"][step0][1:] == -1).all())
        assert bool((dead["finished"][step0] == 1).all())


# ---------------------------------------------------------------- 2. / 3. the oracle search and the conditions of the GPU comparison
def test_oracle_search_without_rules_is_the_known_one():
    from t2s_beam_guided_restated import oracle_beam_guided
    g, sd = load_small("cosingle_small")
    src = torch.from_numpy(g["source_ids"])[:, :9]
    for scale, ref in ((1.0, br.oracle_beam(sd, src, 2, 10)), (2.0, oracle_beam_guided(sd, src, 2, 10, 2.0))):
        got = rr.oracle_beam(sd, src, 2, 10, 0, 0, scale)
        assert [s["hyps"] for s in got] == [s["hyps"] for s in ref] and [s["margin"] for s in got] == [s["margin"] for s in ref]
        assert [s["bound"] for s in got] == [s["bound"] for s in ref] and not any(s["differs"] for s in got)


@pytest.mark.parametrize("case", rr.ORACLE_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_oracle_cases_meet_their_conditions(case):
    """Measured with the fp64 oracle alone: decidable prefixes of 13, 16, 12 and 17 steps; the rules change the selection at 10, 8, 3 and 7
    of them, and 13, 15, 11 and 13 re-parent."""
    name, ids, B, n, m, scale = case
    g, sd = load_small(name)
    steps, k, acc, differs, moved = rr.oracle_case(sd, torch.from_numpy(g["source_ids"]), case)
    print(f"{case}: decidable prefix {k} of {len(steps)} steps; the rules change the selection at {differs}, {moved} re-parent")
    assert k >= 12 and differs >= 1 and moved >= 1
    V = sd["semantic_token_emb.weight"].shape[0]
    for t, s in enumerate(steps):                                        # the oracle search itself keeps the rules
        for pre, c, fin, _ in s["hyps"]:
            if c > -math.inf:
                st = torch.tensor([list(x) for x in pre]).T
                assert rr.repeats(st, n) == 0 and not bool((st[:, :m] == V - 1).any())


# ---------------------------------------------------------------- 4. host plumbing
def test_check_beam_rules_and_rows():
    from covomix_amd.t2s import check_beam_rules, rules_active, rules_rows
    assert check_beam_rules(2, 40) == [(1.0, 0, 0, 0)] * 2 and not rules_active(check_beam_rules(2, 40))
    assert check_beam_rules(2, 40, no_repeat_ngram_size=3, min_length=9) == [(1.0, 0, 3, 9)] * 2
    mix = check_beam_rules(3, 40, no_repeat_ngram_size=[0, 2, 8], min_length=5)
    assert mix == [(1.0, 0, 0, 5), (1.0, 0, 2, 5), (1.0, 0, 8, 5)]
    assert check_beam_rules(2, 40, no_repeat_ngram_size=2, min_length=torch.tensor([0, 40])) == [(1.0, 0, 2, 0), (1.0, 0, 2, 40)]
    rows = rules_rows(mix)
    assert rows.dtype == torch.int32 and rows.shape == (3, 4)
    assert rows[:, 0].view(torch.float32).tolist() == [1.0] * 3 and rows[:, 1].tolist() == [0] * 3
    assert rows[:, 2].tolist() == [0, 2, 8] and rows[:, 3].tolist() == [5] * 3
    for bad in (dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=-1), dict(min_length=41), dict(min_length=-1),
                dict(no_repeat_ngram_size=[2]), dict(min_length=[1, 2, 3]), dict(no_repeat_ngram_size=[2, 9]), dict(min_length=1.5),
                dict(no_repeat_ngram_size=True), dict(repetition_window=-1)):
        with pytest.raises(ValueError):
            check_beam_rules(2, 40, **bad)
    with pytest.raises(ValueError, match="beam search"):
        check_beam_rules(2, 40, repetition_penalty=1.3, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="beam search"):
        check_beam_rules(2, 40, repetition_window=4, no_repeat_ngram_size=2)


def test_signatures_and_parser():
    from covomix_amd import generation
    from covomix_amd.conditional_model import CoVoMixModel
    from covomix_amd.t2s import TextToSemanticDecoder
    for fn in (TextToSemanticDecoder.generate_beam, TextToSemanticDecoder.generate_beam_many, CoVoMixModel.synthesis_sample_text2semantic):
        assert inspect.signature(fn).parameters["beam_rules"].default is False, fn
    p = generation.build_parser()
    kw = generation.t2s_sampling_kwargs(p.parse_args(["--t2s_beam_size", "4", "--t2s_beam_rules", "--t2s_no_repeat_ngram", "2",
                                                      "--t2s_min_length", "9"]))
    assert kw == dict(beam_search_decode=True, beam_size=4, beam_rules=True, no_repeat_ngram_size=2, min_length=9)
    assert generation.t2s_sampling_kwargs(p.parse_args(["--t2s_beam_size", "4", "--t2s_beam_rules"])) == \
        dict(beam_search_decode=True, beam_size=4, beam_rules=True)
    with pytest.raises(ValueError, match="t2s_beam_size"):                                  # without the switch: as before
        generation.t2s_sampling_kwargs(p.parse_args(["--t2s_beam_size", "4", "--t2s_no_repeat_ngram", "2"]))
    for flag, v in (("--t2s_repetition_penalty", "1.3"), ("--t2s_repetition_window", "4")):
        with pytest.raises(ValueError, match="t2s_beam_size"):
            generation.t2s_sampling_kwargs(p.parse_args(["--t2s_beam_size", "4", "--t2s_beam_rules", flag, v]))
    assert "beam_rules" not in generation.t2s_sampling_kwargs(p.parse_args(["--t2s_beam_rules"]))      # no beam search: the flag adds nothing


def test_header_binding_and_symbols():
    from covomix_amd import _lib
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "covomix_hip.h")).read())
    assert "#define CVX_ABI_VERSION 113" in hdr and _lib.ABI_VERSION == 113
    assert ("int cvx_t2s_beam_rules_steps(const cvx_t2s_decoder* dec, const cvx_t2s_beam* beam, const cvx_t2s_beam_queue* bq "
            "/* NULL: lock-step */, const cvx_t2s_rules* rules, int32_t n_steps, cvx_stream_t stream);") in hdr
    assert ("int cvx_t2s_beam_select_rules_f32(const float* logits, const float* scores_in, const uint8_t* finished_in, "
            "const int32_t* history, const int32_t* hist_len, const void* table, int32_t groups, int32_t beam_size, int32_t streams, "
            "int32_t V, int32_t hist_ld, int32_t* parents, int64_t* tokens, float* token_lp, float* scores_out, uint8_t* finished_out, "
            "cvx_stream_t stream);") in hdr
    for words in ("The bans are applied AFTER it, as -inf on lp", "one row per UTTERANCE", "beam search has no repetition penalty",
                  "the n-gram bans of that stream are void for this step"):
        assert words in hdr, words
    res, args = _lib.SIGNATURES["cvx_t2s_beam_rules_steps"]
    assert res is C.c_int and args == [C.POINTER(_lib.T2SDecoder), C.POINTER(_lib.T2SBeam), C.POINTER(_lib.T2SBeamQueue),
                                       C.POINTER(_lib.T2SRules), C.c_int32, C.c_void_p]
    res, args = _lib.SIGNATURES["cvx_t2s_beam_select_rules_f32"]
    assert res is C.c_int and args == [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p] * 6
    lib = _lib.load()
    assert lib.cvx_version() == 113 and lib.cvx_t2s_beam_rules_steps and lib.cvx_t2s_beam_select_rules_f32


def test_new_kernels_use_no_scratch():
    from covomix_amd import _lib
    from test_attention_form_d import _gfx950_kernel_descriptors
    sym = re.compile(r"_ZN12_GLOBAL__N_1\d+(beam_shortlist_rules_kernel|beam_shortlist_guided_rules_kernel|beam_merge_rules_kernel|"
                     r"beam_merge_queue_rules_kernel|beam_merge_guided_rules_kernel|beam_merge_guided_queue_rules_kernel|"
                     r"beam_select_rules_kernel)([EI].*)")
    found = {}
    for name, (group, private, vgprs) in _gfx950_kernel_descriptors(_lib.LIB_PATH).items():
        m = sym.fullmatch(name)
        if m:
            print(f"FIGURE {name[:80]}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
            found.setdefault(m.group(1), []).append((group, private))
    assert {k: len(v) for k, v in found.items()} == {
        "beam_shortlist_rules_kernel": 2, "beam_shortlist_guided_rules_kernel": 2, "beam_merge_rules_kernel": 1,
        "beam_merge_queue_rules_kernel": 1, "beam_merge_guided_rules_kernel": 1, "beam_merge_guided_queue_rules_kernel": 1,
        "beam_select_rules_kernel": 1}, found
    assert all(private == 0 and group <= 64 * 1024 for v in found.values() for group, private in v), found
