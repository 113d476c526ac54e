"""CPU: the host side of the ragged prompt-mel call (mel.extract_mel_many / cvx_mel_spectrogram_many_f32) - the item table against
a Python restatement (tests/mel_items.py), the layout's promises checked on the table itself, every refusal, the batch split, the
ABI additions and the CLI flag.  No GPU is needed: everything here is host arithmetic of the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mel_items
from conftest import ROOT

SYMBOLS = ("cvx_mel_items_words", "cvx_mel_items_fill", "cvx_mel_pack_f32", "cvx_mel_log_gather_f32", "cvx_mel_workspace_bytes_many",
           "cvx_mel_spectrogram_many_f32")
GEOMETRIES = [(480, 160), (1024, 256), (320, 160)]
EINVAL = -22


def length_lists(n_fft, hop):
    """The three lists: one item of pad + 1 samples, the edges around one and two windows, 40 seeded random lengths in [161, 20000].
    (320, 160) has pad = 80: the lists of the default geometry are legal there and take 100 and 90 as well, for T_b = 0.
    (1024, 256) has pad = 384, where 161 ... 384 samples are refused (test_illegal_batches_are_refused): its lists are the same edges
    expressed in its own pad, hop and n_fft, and random lengths in [385, 20000]."""
    pad = (n_fft - hop) // 2
    rng = np.random.RandomState(n_fft + hop)
    rand = [int(v) for v in rng.randint(max(161, pad + 1), 20001, size=40)]
    if (n_fft, hop) == (480, 160):
        return [[161], [161, 319, 320, 479, 480, 481, 25440, 16123], rand]
    if (n_fft, hop) == (320, 160):
        return [[161, 100, 90], [161, 319, 320, 479, 480, 481, 25440, 16123, 100, 90], rand[:20] + [100, 90] + rand[20:38]]
    return [[pad + 1], [pad + 1, 2 * hop - 1, 2 * hop, n_fft - 1, n_fft, n_fft + 1, 159 * hop, 16123], rand]


CASES = [(g, i) for g in GEOMETRIES for i in range(3)]


@pytest.mark.parametrize("geometry,which", CASES)
def test_item_table_against_a_python_restatement(geometry, which):
    from covomix_amd import mel
    n_fft, hop = geometry
    lengths = length_lists(n_fft, hop)[which]
    tab = mel.mel_item_table(lengths, n_fft=n_fft, hop=hop)
    want = mel_items.item_table(lengths, n_fft, hop)
    assert want is not None and tab.words.dtype == np.int32
    assert np.array_equal(tab.words, want)
    assert [int(t) for t in tab.frames] == [mel_items.frames(n, n_fft, hop) for n in lengths]
    if geometry == (480, 160):
        assert [int(t) for t in tab.frames] == [n // 160 for n in lengths]
    if geometry == (320, 160):
        assert sum(int(t) == 0 for t in tab.frames) >= 2               # 100 and 90: pad < n_b, padded item shorter than n_fft


@pytest.mark.parametrize("geometry,which", CASES)
def test_valid_rows_read_their_own_item_and_items_do_not_overlap(geometry, which):
    from covomix_amd import mel
    n_fft, hop = geometry
    lengths = length_lists(n_fft, hop)[which]
    tab = mel.mel_item_table(lengths, n_fft=n_fft, hop=hop)
    pad = tab.pad
    assert pad == (n_fft - hop) // 2 and tab.n == len(lengths)
    end = 0
    for b, n in enumerate(lengths):
        S = int(tab.slot[b]) * hop
        assert S % hop == 0 and S >= end, "an item starts inside the item before"
        if b:
            assert int(tab.slot[b]) == -(-end // hop), "the next item starts at the next slot"
        end = S + n + 2 * pad                                           # the item's padded span is [S, end)
        for t in (range(int(tab.frames[b])) if tab.frames[b] < 8 else (0, 1, int(tab.frames[b]) - 2, int(tab.frames[b]) - 1)):
            r0 = (int(tab.slot[b]) + t) * hop                           # global row slot_b + t reads [r0, r0 + n_fft)
            assert S <= r0 and r0 + n_fft <= end
        assert int(tab.cu[b]) == sum(int(v) for v in tab.frames[:b])
        assert int(tab.raw_off[b]) % 4 == 0 and (b == 0 or int(tab.raw_off[b]) >= int(tab.raw_off[b - 1]) + lengths[b - 1])
    assert tab.rows == -(-end // hop) and tab.M == int(tab.frames.sum()) and tab.max_T == int(tab.frames.max())
    assert tab.packed_floats == -(-(tab.rows * hop + n_fft - hop) // 4) * 4
    assert (tab.rows - 1) * hop + n_fft <= tab.packed_floats           # the last row of the strided view stays inside the buffer


def test_item_table_with_filter_banks():
    """Items of other source rates: n_b = ceil(up * n_raw / down), bank records behind the items."""
    from covomix_amd import hubert, mel
    rates = [16000, 44100, 4000]
    geoms = [mel_items.bank_geometry(r, 8000) for r in rates]
    for r, g in zip(rates, geoms):
        kern, width, orig, new = hubert.sinc_resample_kernel(r, 8000)
        assert g == (new, orig, width) and kern.shape == (new, 2 * width + orig)
    n_raw = [8000, 16001, 44100 + 7, 4000, 12345, 900]
    bank = [-1, 0, 1, 2, 0, 1]
    tab = mel.mel_item_table(n_raw, bank, geoms)
    want = mel_items.item_table(n_raw, 480, 160, bank, geoms)
    assert np.array_equal(tab.words, want)
    assert [int(v) for v in tab.samples] == [8000, 8001, 8002, 8000, 6173, 164]
    assert tab.n_banks == 3 and tab.bank_floats == sum(g[0] * (2 * g[2] + g[1]) for g in geoms)


def _raw_call(n_fft, hop, n_raw, bank=None, geoms=(), words=None):
    """(cvx_mel_items_words, cvx_mel_items_fill's return code, the table as the call left it)"""
    from covomix_amd import _lib
    lib = _lib.load()
    ns = np.asarray(n_raw, dtype=np.int64)
    bk = np.asarray(bank if bank is not None else [-1] * len(n_raw), dtype=np.int32)
    gm = np.asarray(geoms, dtype=np.int32).reshape(-1, 3)
    args = (n_fft, hop, ns.ctypes.data if len(ns) else None, bk.ctypes.data if len(bk) else None, gm.ctypes.data if len(gm) else None,
            len(gm), len(n_raw))
    count = int(lib.cvx_mel_items_words(*args))
    table = np.full(words if words is not None else max(count, 64), -7, dtype=np.int32)
    return count, int(lib.cvx_mel_items_fill(*args, table.ctypes.data, table.size)), table


@pytest.mark.parametrize("what,n_fft,hop,n_raw,bank,geoms", [
    ("no items", 480, 160, [], None, ()),
    ("n_b == pad", 480, 160, [8000, 160, 8000], None, ()),
    ("n_b < pad", 480, 160, [159], None, ()),
    ("n_b == pad through a bank", 480, 160, [320], [0], [(1, 2, 13)]),
    ("n_fft no multiple of 4", 482, 160, [8000], None, ()),
    ("hop no multiple of 4", 480, 162, [8000], None, ()),
    ("hop larger than n_fft", 160, 480, [8000], None, ()),
    ("packed size beyond int32", 480, 160, [(1 << 30) - 8, (1 << 30) - 8, 4096], None, ()),
    ("bank that the call does not have", 480, 160, [8000], [1], [(1, 2, 13)]),
    ("bank below -1", 480, 160, [8000], [-2], ()),
    ("negative sample count", 480, 160, [8000, -1], None, ()),
    ("2^24 frames", 4, 4, [1 << 26, 16], None, ()),
])
def test_illegal_batches_are_refused(what, n_fft, hop, n_raw, bank, geoms):
    count, rc, table = _raw_call(n_fft, hop, n_raw, bank, geoms)
    assert count == -1, what
    assert rc == EINVAL, what
    assert (table == -7).all(), "a refused fill wrote into the table"
    assert mel_items.item_table(n_raw, n_fft, hop, bank, list(geoms)) is None, "the restatement accepts it"


def test_fill_refuses_a_table_that_is_too_small_and_zero_frame_items_are_legal():
    count, rc, table = _raw_call(320, 160, [100, 500, 90, 321, 100])
    assert count == 16 + 8 * 5 and rc == 0
    assert table[16:16 + 40].reshape(5, 8)[:, 4].tolist() == [0, 3, 0, 2, 0]
    _, rc, small = _raw_call(320, 160, [100, 500, 90, 321, 100], words=count - 1)
    assert rc == EINVAL and (small == -7).all()


def test_a_table_that_was_tampered_with_is_refused_before_anything_runs():
    """The calls re-derive the host table from its own words: every changed word is refused (no GPU is reached - the check comes first)."""
    from covomix_amd import _lib, mel
    lib = _lib.load()
    tab = mel.mel_item_table([161, 8000, 700], [-1, 0, -1], [(1, 2, 13)])
    w = tab.words
    assert lib.cvx_mel_workspace_bytes_many(w.ctypes.data, w.size, 3, 80) > 0
    assert lib.cvx_mel_workspace_bytes_many(w.ctypes.data, w.size, 2, 80) == -1          # another item count
    assert lib.cvx_mel_workspace_bytes_many(w.ctypes.data, w.size - 1, 3, 80) == -1      # another word count
    assert lib.cvx_mel_workspace_bytes_many(w.ctypes.data, w.size, 3, 0) == -1
    dummy = np.zeros(64, dtype=np.float32)
    for i in range(w.size):
        bad = w.copy()
        bad[i] += 1
        assert lib.cvx_mel_workspace_bytes_many(bad.ctypes.data, bad.size, 3, 80) == -1, f"word {i}"
        p = dummy.ctypes.data
        assert lib.cvx_mel_spectrogram_many_f32(p, p, p, p, 80, bad.ctypes.data, p, bad.size, 3, p, p, 1 << 30, None) == EINVAL, f"word {i}"
        assert lib.cvx_mel_pack_f32(p, p, bad.ctypes.data, p, bad.size, 3, p, None) == EINVAL
        assert lib.cvx_mel_log_gather_f32(p, bad.ctypes.data, p, bad.size, 3, 80, p, None) == EINVAL
    assert (dummy == 0).all()


def test_workspace_covers_every_buffer_of_the_call():
    from covomix_amd import _lib, mel
    tab = mel.mel_item_table([161, 8000, 700])
    need = _lib.load().cvx_mel_workspace_bytes_many(tab.words.ctypes.data, tab.words.size, 3, 80)
    floats = tab.packed_floats + tab.rows * (2 * 241 + 244 + 80)
    assert 4 * floats <= need <= 4 * floats + 4 * 256


def test_split_batches():
    from covomix_amd import mel
    size = lambda n: -(-(n + 320) // 160) * 160                          # reflect padded, rounded up to the hop
    assert mel.split_batches([], 1000) == []
    assert mel.split_batches([8000, 8000, 8000], 10 ** 9) == [[0, 1, 2]]
    assert size(8000) == 8320
    assert mel.split_batches([8000] * 5, 2 * 8320) == [[0, 1], [2, 3], [4]]
    assert mel.split_batches([8000] * 5, 2 * 8320 - 1) == [[0], [1], [2], [3], [4]]
    assert mel.split_batches([8000, 100000, 161, 161], 20000) == [[0], [1], [2, 3]]           # an item above the budget stands alone
    assert mel.split_batches([1000, 1000], 2 * 1280, n_fft=320, hop=160) == [[0, 1]]          # 1000 + 160 -> 1280
    assert mel.split_batches([1000, 1000], 2 * 1280 - 1, n_fft=320, hop=160) == [[0], [1]]
    groups = mel.split_batches(list(range(200, 4000, 37)), 30000)
    assert [i for g in groups for i in g] == list(range(len(range(200, 4000, 37))))
    assert all(sum(size(200 + 37 * i) for i in g) <= 30000 for g in groups)


def test_header_binding_and_version():
    from covomix_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "covomix_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int(64_t)?\s+" + name + r"\s*\(", hdr, re.M), f"{name} has no prototype in the header"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CVX_ABI_VERSION 113" in hdr and lib.cvx_version() == 113 and _lib.ABI_VERSION == 113
    assert _lib.SIGNATURES["cvx_mel_items_words"][0] is C.c_int64 and _lib.SIGNATURES["cvx_mel_workspace_bytes_many"][0] is C.c_int64


def test_python_entry_points_without_a_gpu():
    from covomix_amd import _lib, mel
    assert mel.mel_spectrogram_many([]) == [] and mel.extract_mel_many([]) == []
    with pytest.raises(NotImplementedError):
        mel.mel_spectrogram_many([], center=True)
    with pytest.raises(NotImplementedError):
        mel.extract_mel_many([np.zeros(800, np.float32)], win_size=400)
    with pytest.raises(ValueError):
        mel.extract_mel_many([np.zeros(800, np.float32)], n_fft=482, win_size=482)
    with pytest.raises(_lib.CovomixHipError):
        mel.mel_spectrogram_many([torch.zeros(800)])                                          # a CPU tensor: there is no CPU path
    with pytest.raises(_lib.CovomixHipError):
        mel.extract_mel_many([np.zeros(800, np.float32)], device="cpu")
    with pytest.raises(ValueError, match="item 1 "):
        mel.extract_mel_many([np.zeros(800, np.float32), np.zeros(160, np.float32)])          # n_b == pad
    with pytest.raises(ValueError, match="2 channel indices"):
        mel.extract_mel_many([np.zeros(800, np.float32)], channel_idx=[0, 1])
    with pytest.raises(TypeError):
        mel.extract_mel_many([np.zeros(800, np.float32)], hop=160)


def test_mel_batch_flag_parses_and_defaults_to_1():
    from covomix_amd import generation
    p = generation.build_parser()
    assert p.parse_args([]).mel_batch == 1
    assert p.parse_args(["--mel_batch", "16"]).mel_batch == 16


def test_prepass_fills_the_dict_load_prompt_consults(tmp_path, monkeypatch):
    """The pre-pass asks extract_mel_many for the prompts without a .mel.npy only, in groups of N, and _load_prompt takes them."""
    from covomix_amd import generation, mel
    calls = []

    def fake(paths):
        calls.append([os.path.basename(p) for p in paths])
        return [torch.full((80, 5), float(len(calls))) for _ in paths]
    monkeypatch.setattr(mel, "extract_mel_many", fake)
    monkeypatch.setattr(generation, "_PROMPT_MELS", {})
    monkeypatch.setattr(generation, "_HUBERT", None)
    d = str(tmp_path)
    for name in ("p1", "p2", "p3", "p4"):
        np.save(str(tmp_path / f"{name}.hubert_code.npy"), np.arange(5))
    np.save(str(tmp_path / "p2.mel.npy"), np.zeros((80, 5), dtype=np.float32))
    assert generation.preextract_prompt_mels(d, ["p1", "p2", "p3", "p1", "p4"], 2) == 3
    assert calls == [["p1.wav", "p3.wav"], ["p4.wav"]]
    assert float(generation._load_prompt(d, "p4")[1].max()) == 2.0
    assert float(generation._load_prompt(d, "p2")[1].abs().max()) == 0.0                      # a mel file on disk still wins
