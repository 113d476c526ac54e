"""CPU: the host side of guided and unguided utterances in one slot pool (cvx_t2s_decode_steps_mixed, generate_many(mixed_guidance=True)):
check_settings(mixed=True), the record layout and the window cut, the scheduler policy replayed on the host (mixed_schedule) on
hand-worked cases, and the C struct / signature as the header and _lib.py see them."""
import ctypes as C
import math
import os
import re

import pytest

from conftest import ROOT


def test_check_settings_mixed():
    from covomix_amd.t2s import check_settings
    V = 100
    got = check_settings([{"cond_scale": 1.0}, {"cond_scale": 2.0}, {"cond_scale": 1.0}], 3, V, mixed=True)
    assert [r[2] for r in got] == [1.0, 2.0, 1.0]
    # the call's cond_scale is only the default
    got = check_settings([None, {"cond_scale": 1.0}, {"cond_scale": 3.0, "temperature": 0.5}], 3, V, cond_scale=1.5, mixed=True)
    assert [r[2] for r in got] == [1.5, 1.0, 3.0] and got[2][0] == 0.5
    for bad in (0.5, math.nan, 0.0, -2.0):
        with pytest.raises(ValueError, match="cond_scale"):
            check_settings([None, {"cond_scale": bad}], 2, V, mixed=True)
    with pytest.raises(ValueError, match="cond_scale"):
        check_settings([None], 1, V, cond_scale=0.5, mixed=True)
    # two-output models: all scales 1 are fine, any scale > 1 is not
    assert len(check_settings([None, {"cond_scale": 1.0}], 2, V, streams=2, mixed=True)) == 2
    with pytest.raises(NotImplementedError):
        check_settings([None, {"cond_scale": 2.0}], 2, V, streams=2, mixed=True)
    with pytest.raises(NotImplementedError):
        check_settings([None], 1, V, streams=2, cond_scale=2.0, mixed=True)
    # whatever else check_settings refuses stays refused
    with pytest.raises(ValueError):
        check_settings([{"temperature": -1.0}], 1, V, mixed=True)
    with pytest.raises(ValueError):
        check_settings([None], 2, V, mixed=True)


def test_check_settings_without_mixed_is_unchanged():
    from covomix_amd.t2s import check_settings
    V = 100
    with pytest.raises(ValueError, match="two calls"):
        check_settings([None, {"cond_scale": 2.0}], 2, V)
    with pytest.raises(ValueError, match="two calls"):
        check_settings([None, {"cond_scale": 1.0}], 2, V, cond_scale=1.5)
    with pytest.raises(ValueError, match="two calls"):
        check_settings([None, {"cond_scale": 2.0}], 2, V, mixed=False)
    with pytest.raises(NotImplementedError):
        check_settings([None], 1, V, streams=2, cond_scale=2.0)
    assert [r[2] for r in check_settings([None, {"cond_scale": 3.0}], 2, V, cond_scale=1.5)] == [1.5, 3.0]


def test_record_layout_and_windows():
    from covomix_amd.t2s import WINDOW, mixed_records, mixed_windows
    assert mixed_records([]) == [0]
    assert mixed_records([False, True, True, False]) == [0, 1, 3, 5, 6]
    assert mixed_records([True, False]) == [0, 2, 3]
    assert WINDOW == 256
    assert mixed_windows([False] * 256) == [(0, 256)]
    assert mixed_windows([True] * 128) == [(0, 128)]
    assert mixed_windows([False] * 257) == [(0, 256), (256, 257)]
    # 200 guided + 1 unguided: 401 records; no pair is cut
    kinds = [True] * 200 + [False]
    wins = mixed_windows(kinds)
    assert wins == [(0, 128), (128, 201)]
    # an unguided utterance first shifts every pair by one record: the first window ends one record short rather than cut a pair
    kinds = [False] + [True] * 200
    wins = mixed_windows(kinds)
    assert wins == [(0, 128), (128, 201)]
    for kinds in ([False] + [True] * 200, [True, False, False] * 150, [True] * 129):
        wins = mixed_windows(kinds)
        assert wins[0][0] == 0 and wins[-1][1] == len(kinds) and all(a[1] == b[0] for a, b in zip(wins, wins[1:]))
        for a, b in wins:
            assert 0 < mixed_records(kinds[a:b])[-1] <= WINDOW
    assert mixed_windows([True, True, False], window=3) == [(0, 1), (1, 3)]
    assert mixed_windows([]) == []


def test_mixed_schedule_hand_worked():
    from covomix_amd.t2s import mixed_schedule
    G, U = True, False
    # a guided head waits for a second slot: 3 slots, U U U then G; the unguided ones end after 2, 5 and 7 steps.  After step 2 one slot
    # is idle - the guided head waits; after step 5 slots 0 and 1 are idle and it takes both
    assert mixed_schedule([U, U, U, G], [2, 5, 7, 3], 3) == [(0, None, 0), (1, None, 0), (2, None, 0), (0, 1, 5)]
    # ... and it blocks what is behind it (strict order): the unguided utterance behind the head does not overtake into the idle slot
    assert mixed_schedule([U, U, U, G, U], [2, 5, 7, 3, 1], 3) == [(0, None, 0), (1, None, 0), (2, None, 0), (0, 1, 5), (2, None, 7)]
    # partners that are not neighbours: slots 0 and 2 idle while slot 1 still decodes
    assert mixed_schedule([U, U, U, G], [2, 9, 2, 4], 3) == [(0, None, 0), (1, None, 0), (2, None, 0), (0, 2, 2)]
    # a guided utterance behind the first step's hand-out: one idle slot is not enough, it starts when the unguided one has ended
    assert mixed_schedule([G, U, G], [4, 1, 2], 4) == [(0, 1, 0), (2, None, 0), (2, 3, 1)]
    # an odd tail record is never taken: the second record of the last guided utterance lies beyond the queue's count
    assert mixed_schedule([U, G], [1, 1], 4, n_records=2) == [(0, None, 0), None]
    assert mixed_schedule([G, U], [1, 1], 4, n_records=1) == [None, None]
    assert mixed_schedule([U, G], [1, 1], 4, n_records=3) == [(0, None, 0), (1, 2, 0)]
    # slots = 2 with alternating kinds drains: one utterance at a time whenever a guided one is involved
    got = mixed_schedule([G, U, G, U, U, G], [3, 2, 1, 4, 2, 5], 2)
    assert got == [(0, 1, 0), (0, None, 3), (0, 1, 5), (0, None, 6), (1, None, 6), (0, 1, 10)]
    # more slots than records, and a single unguided slot
    assert mixed_schedule([U, G], [3, 3], 8) == [(0, None, 0), (1, 2, 0)]
    assert mixed_schedule([U, U], [3, 2], 1) == [(0, None, 0), (0, None, 3)]
    # a guided head that can never get two slots is never taken, nor what is behind it
    assert mixed_schedule([U, G, U], [2, 2, 2], 1) == [(0, None, 0), None, None]
    with pytest.raises(ValueError):
        mixed_schedule([U], [0], 2)
    with pytest.raises(ValueError):
        mixed_schedule([U, G], [1], 2)


def test_public_signatures():
    import inspect
    from covomix_amd.t2s import TextToSemanticDecoder
    sig = inspect.signature(TextToSemanticDecoder.generate_many)
    assert sig.parameters["mixed_guidance"].default is False
    assert "mixed_guidance" in inspect.signature(TextToSemanticDecoder.score_many).parameters


def test_struct_and_signature_agree_with_the_header():
    from covomix_amd import _lib
    with open(os.path.join(ROOT, "include", "covomix_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"typedef struct cvx_t2s_mixed \{(.*?)\} cvx_t2s_mixed;", hdr, re.S)
    assert m, "cvx_t2s_mixed is not declared in the header"
    fields = re.findall(r"(\w+)\s+(\w+);", m.group(1))
    assert fields == [("uint32_t", "struct_size"), ("int32_t", "n_guided")]
    assert [f[0] for f in _lib.T2SMixed._fields_] == ["struct_size", "n_guided"]
    assert C.sizeof(_lib.T2SMixed) == 8 and _lib.T2SMixed.n_guided.offset == 4
    ret, args = _lib.SIGNATURES["cvx_t2s_decode_steps_mixed"]
    assert ret is C.c_int and args == [C.POINTER(_lib.T2SDecoder), C.POINTER(_lib.T2SScoring), C.POINTER(_lib.T2SPerDialogue),
                                       C.POINTER(_lib.T2SMixed), C.c_int32, C.c_void_p]
    assert re.search(r"int cvx_t2s_decode_steps_mixed\(const cvx_t2s_decoder\* dec, const cvx_t2s_scoring\* scoring, "
                     r"const cvx_t2s_per_dialogue\* per,\s+const cvx_t2s_mixed\* mixed, int32_t n_steps, cvx_stream_t stream\);", hdr)
    assert re.search(r"#define CVX_T2S_FLAG_GUIDED 4\b", hdr) and _lib.T2S_FLAG_GUIDED == 4
    assert re.search(r"#define CVX_ABI_VERSION 113\b", hdr) and _lib.ABI_VERSION == 113
    assert hasattr(_lib.load(), "cvx_t2s_decode_steps_mixed")


def test_cli_flag_becomes_a_keyword():
    from covomix_amd import generation
    base = ["--acous_ckpt", "a", "--hifigan_ckpt", "h", "--text_dir", "t", "--prompt_dir", "p", "--saved_dir", "s"]
    off = generation.build_parser().parse_args(base)
    on = generation.build_parser().parse_args(base + ["--t2s_mixed_guidance"])
    assert off.t2s_mixed_guidance is False and "mixed_guidance" not in generation.t2s_sampling_kwargs(off)
    assert generation.t2s_sampling_kwargs(on) == {"mixed_guidance": True}
