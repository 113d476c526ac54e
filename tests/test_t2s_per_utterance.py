"""CPU: per-utterance sampling settings and forced prefixes of the text2semantic decode - what the host accepts and refuses before
anything reaches the device (t2s.check_settings, t2s.check_prefixes), the bits of the settings table it writes (t2s.settings_rows)
and the C struct of cvx_t2s_decode_steps_per_dialogue as the header and _lib.py see it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 503


def test_check_settings_resolves_against_the_scalars():
    from covomix_amd import _lib
    from covomix_amd.t2s import UtteranceSettings, check_settings, filter_setting
    res = check_settings([None, {"temperature": 0.7}, {"filter_logits_fn": "top_p", "filter_fn_kwargs": {"thres": 0.5}},
                          UtteranceSettings(filter_fn_kwargs={"k": 7}), {"temperature": 0, "filter_logits_fn": "top_p"}, {}],
                         6, V, 1, temperature=1.3, filter_logits_fn="top_k", filter_fn_kwargs={"thres": 0.2})
    default = filter_setting("top_k", {"thres": 0.2}, V)
    assert res[0] == (1.3, default, 1.0) and res[5] == res[0]
    assert res[1] == (0.7, default, 1.0)
    assert res[2] == (1.3, (_lib.T2S_FILTER_TOP_P, 0, 0.5), 1.0)
    assert res[3] == (1.3, (_lib.T2S_FILTER_TOP_K, 7, 0.0), 1.0)
    assert res[4] == (0.0, (_lib.T2S_FILTER_TOP_P, 0, 0.9), 1.0)           # (another filter: its own defaults, not the call's top_k kwargs)
    guided = check_settings([{"cond_scale": 2.0}, None, {"cond_scale": 3.0, "temperature": 0.5}], 3, V, 1, cond_scale=1.5)
    assert [r[2] for r in guided] == [2.0, 1.5, 3.0] and guided[2][0] == 0.5
    assert check_settings([], 0, V) == []


def test_check_settings_refusals():
    from covomix_amd.t2s import check_settings
    with pytest.raises(ValueError, match="2 entries for 3"):
        check_settings([None, None], 3, V)
    for bad in ({"temperature": -0.1}, {"temperature": float("nan")}, {"temprature": 1.0}, {"filter_logits_fn": "top_a"},
                {"filter_fn_kwargs": {"k": 0}}, {"filter_fn_kwargs": {"k": V + 1}}, {"filter_fn_kwargs": {"p": 1}},
                {"filter_logits_fn": "top_p", "filter_fn_kwargs": {"thres": 1.0}}, {"filter_logits_fn": "top_p", "filter_fn_kwargs": {"thres": 0.0}},
                {"filter_logits_fn": "top_p", "filter_fn_kwargs": {"k": 3}}):
        with pytest.raises(ValueError):
            check_settings([None, bad], 2, V)
    # guided and unguided utterances do not share a launch
    with pytest.raises(ValueError, match="two calls"):
        check_settings([None, {"cond_scale": 2.0}], 2, V, 1)
    with pytest.raises(ValueError, match="two calls"):
        check_settings([None, {"cond_scale": 0.5}], 2, V, 1)
    with pytest.raises(ValueError, match="two calls"):
        check_settings([{"cond_scale": 2.0}, {"cond_scale": 1.0}], 2, V, 1, cond_scale=2.0)
    with pytest.raises(NotImplementedError):
        check_settings([None], 1, V, 2, cond_scale=2.0)
    with pytest.raises(NotImplementedError):
        check_settings([{"cond_scale": 2.0}], 1, V, 2)
    assert check_settings([{"cond_scale": 1.0}], 1, V, 2)[0][2] == 1.0


def test_table_rows_hold_the_bits_the_scalar_path_computes():
    from covomix_amd import _lib
    from covomix_amd.t2s import check_settings, settings_rows
    temps = [0, 0.0, 1e-12, 1e-10, 0.1, 0.7, 1.0, 1.3, 3.0, 1.0 / 3.0, 123.456]
    sets = [{"temperature": t} for t in temps]
    sets[3] = dict(sets[3], filter_logits_fn="top_p", filter_fn_kwargs={"thres": 0.9})
    sets[4] = dict(sets[4], filter_fn_kwargs={"k": V})
    rows = settings_rows(check_settings(sets, len(sets), V), [0, 3] + [0] * (len(sets) - 2))
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (len(temps), 8) and _lib.T2S_PER_WORDS == 8
    for j, t in enumerate(temps):
        want = np.float32(1) / max(np.float32(t), np.float32(1e-10))
        assert rows[j, 0].item() == int(np.array(want, dtype=np.float32).view(np.int32)), (t, want)
        # ... which is what the C code gets from the descriptor's float: 1.0f / fmaxf((float)t, 1e-10f)
        assert C.c_float(t).value == float(np.float32(t))
    assert rows[0, 0].item() == int(np.array(1e10, dtype=np.float32).view(np.int32))           # T = 0: 1 / 1e-10f
    assert rows[:, 1].tolist() == [0, 0, 0, 1] + [0] * 7
    assert rows[4, 2].item() == V and rows[0, 2].item() == 51                                     # ceil(0.1 * 503)
    assert rows[3, 3].item() == int(np.array(0.9, dtype=np.float32).view(np.int32))
    assert all(x == int(np.array(1.0, dtype=np.float32).view(np.int32)) for x in rows[:, 4].tolist())
    assert rows[:, 5].tolist() == [0, 3] + [0] * 9 and not rows[:, 6:].any()
    g = settings_rows(check_settings([{"cond_scale": 2.5}], 1, V, 1, cond_scale=1.5))
    assert g[0, 4].item() == int(np.array(2.5, dtype=np.float32).view(np.int32))


def test_prefix_checks():
    from covomix_amd.t2s import check_prefixes
    eos = V - 1
    ok = torch.tensor([[1, 2, 3]])
    out = check_prefixes([None, ok, [[5]]], 3, 1, V, [10, 4, 2])
    assert out[0] is None and torch.equal(out[1], ok) and out[1].dtype == torch.int64 and out[2].tolist() == [[5]]
    two = check_prefixes([torch.tensor([[1, 2], [3, 4]], dtype=torch.int32)], 1, 2, V, [5])
    assert tuple(two[0].shape) == (2, 2) and two[0].dtype == torch.int64
    with pytest.raises(ValueError, match="eos"):
        check_prefixes([torch.tensor([[1, eos, 3]])], 1, 1, V, [10])
    with pytest.raises(ValueError, match="nothing to decode"):
        check_prefixes([ok], 1, 1, V, [3])                                 # P == limit
    with pytest.raises(ValueError):
        check_prefixes([torch.tensor([[1, 2, 3, 4]])], 1, 1, V, [3])       # P > limit
    with pytest.raises(ValueError):
        check_prefixes([ok], 1, 2, V, [10])                                # S = 1 tokens for a two-stream model
    with pytest.raises(ValueError):
        check_prefixes([torch.tensor([[1, 2], [3, 4]])], 1, 1, V, [10])
    with pytest.raises(ValueError):
        check_prefixes([torch.zeros(1, 0, dtype=torch.int64)], 1, 1, V, [10])
    with pytest.raises(ValueError):
        check_prefixes([torch.tensor([[V]])], 1, 1, V, [10])
    with pytest.raises(ValueError):
        check_prefixes([torch.tensor([[-1]])], 1, 1, V, [10])
    with pytest.raises(ValueError):
        check_prefixes([torch.tensor([[0.5]])], 1, 1, V, [10])
    with pytest.raises(ValueError, match="forced"):
        check_prefixes([ok, None], 2, 1, V, [10, 10], forced=[torch.tensor([[4, 5]]), None])
    assert check_prefixes([None, ok], 2, 1, V, [10, 10], forced=[torch.tensor([[4, 5]]), None])[1] is not None
    with pytest.raises(ValueError, match="1 entries for 2"):
        check_prefixes([ok], 2, 1, V, [10, 10])


def test_struct_and_signature_agree_with_the_header():
    from covomix_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "covomix_hip.h")).read()
    m = re.search(r"typedef struct cvx_t2s_per_dialogue \{(.*?)\} cvx_t2s_per_dialogue;", hdr, re.S)
    assert m, "cvx_t2s_per_dialogue is not declared in the header"
    fields = [re.sub(r"\s+", " ", f.strip()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["uint32_t struct_size", "int32_t n_records", "const void* table"]
    assert [f[0] for f in _lib.T2SPerDialogue._fields_] == ["struct_size", "n_records", "table"]
    assert C.sizeof(_lib.T2SPerDialogue) == 4 + 4 + 8 == 16
    assert _lib.T2SPerDialogue.n_records.offset == 4 and _lib.T2SPerDialogue.table.offset == 8
    ret, args = _lib.SIGNATURES["cvx_t2s_decode_steps_per_dialogue"]
    assert ret is C.c_int and args == [C.POINTER(_lib.T2SDecoder), C.POINTER(_lib.T2SScoring), C.POINTER(_lib.T2SPerDialogue), C.c_int32,
                                       C.c_void_p]
    assert re.search(r"int cvx_t2s_decode_steps_per_dialogue\(const cvx_t2s_decoder\* dec, const cvx_t2s_scoring\* scoring, "
                     r"const cvx_t2s_per_dialogue\* per,\s+int32_t n_steps, cvx_stream_t stream\);", hdr)
    assert _lib.ABI_VERSION == 113 and "#define CVX_ABI_VERSION 113" in hdr      # a pure addition
    assert hasattr(_lib.load(), "cvx_t2s_decode_steps_per_dialogue")
