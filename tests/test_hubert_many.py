"""CPU: the host side of the ragged HuBERT tokeniser call (many prompts of different lengths in one call): the item table that
cvx_hubert_items_fill writes against a plain Python restatement, the rejection rules, the max_batch_samples split, the batch = 1 code
path of tokenize_directory and the CLI flag.  No GPU: the table is host arithmetic of the library."""
import numpy as np
import pytest

CONV = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2
HOP, HALO = 320, 64


def n(T, r=0):
    """Samples that give T frames for 0 <= r < 320 (receptive field 400, hop 320)."""
    return 320 * (T - 1) + 400 + r


BATCH_A = [n(1, 0), n(1, 245), n(1, 250), n(16, 319), 399, n(17, 1), n(128, 0), n(129, 160), n(37, 7)]
BATCH_B = [n(T) for T in (300, 129, 256, 200, 145)]


def frames(ns, upto=len(CONV)):
    for _c, k, s in CONV[:upto]:
        ns = (ns - k) // s + 1 if ns >= k else 0
    return ns


def restated(lengths):
    """The table's arrays, from the layout rules alone."""
    S, end = [], 0
    for ns in lengths:
        S.append(-(-end // HOP) * HOP)
        end = S[-1] + ns
    T = [frames(ns) for ns in lengths]
    cu = np.concatenate([[0], np.cumsum(T)])
    cuh = cu + 2 * HALO * np.arange(len(lengths) + 1)
    start, rows, div = [], [], 1
    for i, (_c, _k, s) in enumerate(CONV):
        div *= s
        start.append([s0 // div for s0 in S])
        rows.append([frames(ns, i + 1) for ns in lengths])
    chunks = np.concatenate([[0], np.cumsum([-(-r // 128) for r in rows[0]])])
    gather = [S[b] // HOP + t for b in range(len(lengths)) for t in range(T[b])]
    pack_src = []
    for b in range(len(lengths)):
        pack_src += [-1] * HALO + list(range(cu[b], cu[b + 1])) + [-1] * HALO
    unpack = [cuh[b] + t for b in range(len(lengths)) for t in range(T[b])]
    return dict(S=S, end=end, T=T, cu=cu, cuh=cuh, start=start, rows=rows, chunks=chunks, gather=gather, pack_src=pack_src, unpack=unpack)


@pytest.mark.parametrize("lengths", [BATCH_A, BATCH_B, [399], [0, n(3, 5), 9, n(2)], [n(5)]],
                         ids=["batch_a", "batch_b", "one_zero_frame_item", "zero_frame_items_first_and_inside", "single"])
def test_item_table_against_a_python_restatement(lengths):
    from covomix_amd.hubert import item_table
    t, w = item_table(lengths), restated(lengths)
    assert (t.n, t.n_conv, t.hop, t.halo) == (len(lengths), 7, HOP, HALO)
    assert (t.M, t.Mh, t.max_T, t.samples_total) == (sum(w["T"]), sum(w["T"]) + len(lengths) * 128, max(w["T"]), w["end"])
    assert all(int(s) % HOP == 0 for s in t.offsets) and t.offsets.tolist() == w["S"]
    assert t.samples.tolist() == list(lengths) and t.frames.tolist() == w["T"]
    np.testing.assert_array_equal(t.start, np.array(w["start"]))
    np.testing.assert_array_equal(t.rows, np.array(w["rows"]))
    np.testing.assert_array_equal(t.c0, np.stack([w["start"][0], w["rows"][0], w["chunks"][:-1]], 1))
    np.testing.assert_array_equal(t.cu, w["cu"])
    np.testing.assert_array_equal(t.cuh, w["cuh"])
    np.testing.assert_array_equal(t.gather, np.array(w["gather"], dtype=np.int32))
    np.testing.assert_array_equal(t.pack_src, np.array(w["pack_src"], dtype=np.int32))
    np.testing.assert_array_equal(t.unpack, np.array(w["unpack"], dtype=np.int32))
    # a valid row of layer i reads rows of its own item only, and no two items share a row at any layer
    for i in range(7):
        ends = t.start[i] + t.rows[i]
        assert (ends[:-1] <= t.start[i][1:]).all()
        if i:
            k, s = CONV[i][1], CONV[i][2]
            assert ((t.rows[i] == 0) | ((t.rows[i] - 1) * s + k <= t.rows[i - 1])).all()
            assert (t.start[i] * s == t.start[i - 1]).all()


def test_item_table_offsets_of_the_caller_and_rejections():
    from covomix_amd import _lib
    from covomix_amd.hubert import item_table
    t = item_table([n(2), n(3)], offsets=[640, 3200])
    assert t.offsets.tolist() == [640, 3200] and t.start[0].tolist() == [128, 640] and t.gather.tolist() == [2, 3, 10, 11, 12]
    assert t.samples_total == 3200 + n(3)
    for lengths, offsets in (([], None), ([n(2), n(3)], [0, 100]), ([n(2), n(3)], [0, 640]), ([n(2), n(3)], [3200, 0]),
                             ([n(2)], [-320])):
        with pytest.raises(_lib.CovomixHipError):
            item_table(lengths, offsets=offsets)
    with pytest.raises(_lib.CovomixHipError):                              # 2^31 packed samples (reached before 2^24 frames at hop 320)
        item_table([n(1 << 22)] * 4)
    # 2^24 frames in total: a two-layer stack of hop 1 (frames = samples - 2) reaches the frame limit far below the sample limit
    import ctypes as C
    from covomix_amd.hubert import _geometry_model
    tiny = [(4, 2, 1), (4, 2, 1)]
    m, lib = _geometry_model(tiny, 2), _lib.load()
    below, at = np.array([(1 << 23) + 2, (1 << 23) + 1], dtype=np.int64), np.array([(1 << 23) + 2] * 2, dtype=np.int64)
    assert int(lib.cvx_hubert_items_words(C.byref(m), below.ctypes.data, 2)) > 0        # 2^24 - 1 frames
    assert int(lib.cvx_hubert_items_words(C.byref(m), at.ctypes.data, 2)) == -1         # 2^24 frames
    with pytest.raises(_lib.CovomixHipError):
        item_table([(1 << 23) + 2, (1 << 23) + 2], conv_layers=tiny, pos_k=2)


def test_workspace_and_call_reject_a_table_that_was_tampered_with():
    """cvx_hubert_workspace_bytes_many re-derives the host table from its offsets and lengths: any other word makes it illegal."""
    import ctypes as C
    from covomix_amd import _lib
    from covomix_amd.hubert import _geometry_model, item_table
    lib = _lib.load()
    m = _geometry_model(CONV, 128)
    m.dim, m.heads, m.pos_groups, m.n_layers = 768, 12, 16, 0
    for i, (c, _k, _s) in enumerate(CONV):
        m.conv_c[i] = c
    t = item_table(BATCH_A)
    good = int(lib.cvx_hubert_workspace_bytes_many(C.byref(m), t.words.ctypes.data, t.n))
    assert good > 0
    assert int(lib.cvx_hubert_workspace_bytes_many(C.byref(m), t.words.ctypes.data, t.n - 1)) == -1
    for word in (4, 16, 16 + 19 * t.n + 1, t.words.size - 1, t.words.size - t.M - 3):   # halo, an offset, cu[1], an unpack row, a halo entry
        bad = t.words.copy()
        bad[word] += 1
        assert int(lib.cvx_hubert_workspace_bytes_many(C.byref(m), bad.ctypes.data, t.n)) == -1, word
        # the call itself returns CVX_EINVAL before it looks at any device pointer (placeholders here) or launches anything
        assert lib.cvx_hubert_extract_features_many(C.byref(m), 256, bad.ctypes.data, 256, t.n, 0, 256, 256, 1 << 40, None) == -22
    assert lib.cvx_hubert_extract_features_many(C.byref(m), 256, t.words.ctypes.data, 256, 0, 0, 256, 256, 1 << 40, None) == -22   # no items


def test_max_batch_samples_splits_where_expected():
    from covomix_amd.hubert import split_batches
    ten_s = 160000
    assert split_batches([ten_s] * 5, 2 * ten_s) == [[0, 1], [2, 3], [4]]
    assert split_batches([ten_s] * 3, 10 * ten_s) == [[0, 1, 2]]
    assert split_batches([ten_s, 5 * ten_s, ten_s], 2 * ten_s) == [[0], [1], [2]]     # an item over the budget goes alone
    assert split_batches([321, 321, 321], 1280) == [[0, 1], [2]]                      # packed size: every item rounded up to the hop
    assert split_batches([320, 320, 320, 320], 1280) == [[0, 1, 2, 3]]
    assert split_batches([], 100) == []


def test_tokenize_directory_batch_1_takes_the_old_path(tmp_path, monkeypatch):
    from covomix_amd import hubert

    calls = []

    class Stub:
        def __init__(self, **kw):
            pass

        def wav2code(self, path, channel_id=1):
            calls.append(("one", path))
            return "1 2 3"

        def wav2code_many(self, paths, channel_id=1):
            calls.append(("many", tuple(paths)))
            return ["4 5"] * len(paths)

    monkeypatch.setattr(hubert, "HubertTokenizer", Stub)
    for name in ("b", "a", "c"):
        (tmp_path / f"{name}.wav").write_bytes(b"")
    assert hubert.tokenize_directory(str(tmp_path), str(tmp_path / "o1"), "ckpt", "km") == 3
    assert [c[0] for c in calls] == ["one"] * 3 and [c[1][-5:] for c in calls] == ["a.wav", "b.wav", "c.wav"]
    assert np.load(str(tmp_path / "o1" / "a.hubert_code.npy")).tolist() == ["1", "2", "3"]
    calls.clear()
    assert hubert.tokenize_directory(str(tmp_path), str(tmp_path / "o2"), "ckpt", "km", batch=2) == 3
    assert [(c[0], len(c[1])) for c in calls] == [("many", 2), ("many", 1)]
    assert np.load(str(tmp_path / "o2" / "c.hubert_code.npy")).tolist() == ["4", "5"]


def test_hubert_batch_flag_parses_and_defaults_to_1():
    from covomix_amd.generation import build_parser, prompt_names
    p = build_parser()
    assert p.parse_args([]).hubert_batch == 1
    assert p.parse_args(["--hubert_batch", "16"]).hubert_batch == 16
    assert prompt_names(["u1", "u2"], True) == ["u1_1", "u1_2", "u2_1", "u2_2"] and prompt_names(["u1"], False) == ["u1"]


def test_prepass_fills_the_dict_load_prompt_consults(tmp_path, monkeypatch):
    from covomix_amd import generation

    class Stub:
        def __init__(self):
            self.calls = []

        def wav2code_many(self, paths, channel_id=1):
            self.calls.append(list(paths))
            return [" ".join(str(len(p) % 7 + i) for i in range(3)) for p in paths]

        def wav2code(self, path, channel_id=1):
            raise AssertionError("the pre-pass already holds this prompt")

    stub = Stub()
    monkeypatch.setattr(generation, "_HUBERT", stub)
    monkeypatch.setattr(generation, "_HUBERT_CODES", {})
    d = str(tmp_path)
    np.save(str(tmp_path / "p2.hubert_code.npy"), np.array(["9", "8"]))
    for name in ("p1", "p2", "p3", "p4"):
        np.save(str(tmp_path / f"{name}.mel.npy"), np.zeros((80, 4), dtype=np.float32))
    assert generation.pretokenise_prompts(d, ["p1", "p2", "p3", "p1", "p4"], 2) == 3
    assert [[p.split("/")[-1] for p in c] for c in stub.calls] == [["p1.wav", "p3.wav"], ["p4.wav"]]
    tok, mel = generation._load_prompt(d, "p3")                       # three codes from the dict, cut to the mel's four frames
    assert tok.tolist() == [int(c) for c in generation._HUBERT_CODES[(d, "p3")].split(" ")] and mel.shape == (3, 80)
    assert generation._load_prompt(d, "p2")[0].tolist() == [9, 8]     # a code file on disk still wins
